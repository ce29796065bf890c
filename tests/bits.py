"""Bit equality of two arrays of doubles: the one comparison every "bit for bit" test uses, on the device and on the host."""
import numpy as np


def same_bits(a, b) -> bool:
    """equal shape, NaN in the same places (whatever its payload), the same bit patterns everywhere else: +0.0 is not -0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(a.view(np.int64)[~np.isnan(a)], b.view(np.int64)[~np.isnan(b)])


def first_difference(a, b) -> str:
    """for an assert's message: where two arrays first differ by same_bits' rule, and the two values there"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    differ = np.argwhere((np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a.view(np.int64) != b.view(np.int64))))
    if not differ.size:
        return "no difference"
    at = tuple(int(i) for i in differ[0])
    return "%d of %d entries differ, the first at %s: %r and %r" % (len(differ), a.size, at, float(a[at]), float(b[at]))
