"""The two rules of the test tree itself: the one same_bits is the strict one, and no file under tests/ imports a test
module -- what test modules share lives in plain helper modules (bits.py, pixel_cases.py, xcor_checks.py,
observed_cases.py and the *_cases.py beside them)."""
import glob
import os
import re

import numpy as np

from bits import same_bits

HERE = os.path.dirname(os.path.abspath(__file__))


def test_same_bits_is_the_strict_one():
    a = np.array([[1.0, 0.0, -2.5], [np.nan, 3.0, np.inf]])
    assert same_bits(a, a.copy())
    # the sign of zero
    assert not same_bits(np.array([0.0]), np.array([-0.0])) and same_bits(np.array([-0.0]), np.array([-0.0]))
    # equal bits, another shape
    assert not same_bits(a, a.reshape(3, 2)) and not same_bits(a, a.ravel())
    # NaN at another place
    assert not same_bits(np.array([np.nan, 1.0]), np.array([1.0, np.nan]))
    assert not same_bits(np.array([np.nan, 1.0]), np.array([0.0, 1.0]))
    # NaN of another payload (and sign) at the same place
    other = a.copy()
    other.view(np.uint64)[1, 0] = np.uint64(0xFFF8000000000123)
    assert np.isnan(other[1, 0]) and other.view(np.uint64)[1, 0] != a.view(np.uint64)[1, 0]
    assert same_bits(a, other)
    # one bit of one entry
    near = a.copy()
    near[0, 2] = np.nextafter(near[0, 2], 0.0)
    assert not same_bits(a, near)
    # non-contiguous input
    wide = np.arange(24.0).reshape(4, 6)
    wide[1, 2], wide[3, 4] = np.nan, -0.0
    assert not wide[::2, 1::2].flags["C_CONTIGUOUS"] and not wide.T.flags["C_CONTIGUOUS"]
    assert same_bits(wide[::2, 1::2], wide[::2, 1::2].copy()) and same_bits(wide.T, wide.T.copy())
    assert not same_bits(wide[::2, 1::2], wide[1::2, 1::2])


def test_no_test_file_imports_a_test_module():
    found = []
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        with open(path) as f:
            for k, line in enumerate(f, 1):
                if re.match(r"\s*(import|from) test_", line):
                    found.append("%s:%d: %s" % (os.path.basename(path), k, line.strip()))
    assert not found, found
