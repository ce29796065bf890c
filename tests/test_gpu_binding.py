"""The calls that need an installed set, on an Engine that has none: each is refused by the library with its own status
(an EngineError, never a ctypes or AttributeError of the binding), and the handle computes the same bits afterwards."""
import numpy as np
import pytest

from cases import golden
from transit_amd import _abi
from transit_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu


def test_calls_without_their_set_are_refused_and_leave_the_handle_as_it_was():
    P = golden("eclipse_small").problem
    eng = Engine(P.static)
    first = eng.run(P.atm, P.opts)["spectrum"]
    one = [1.0]
    # every status below is TRX_E_ARG (-1), as recorded with the hand-written binding this one replaced
    refused = [
        ("run_bands", lambda: eng.run_bands(P.atm, P.opts), -1),
        ("run_pixels", lambda: eng.run_pixels(P.atm, P.opts, one), -1),
        ("run_moments", lambda: eng.run_moments(P.atm, P.opts, one), -1),
        ("run_trail", lambda: eng.run_trail(P.atm, P.opts, one), -1),
        ("run_filtered_moments", lambda: eng.run_filtered_moments(P.atm, P.opts, one), -1),
        ("run_highpassed", lambda: eng.run_highpassed(P.atm, P.opts, one), -1),
        ("run_exposed", lambda: eng.run_exposed(P.atm, P.opts, one), -1),
        ("detrend_observed", lambda: eng.detrend_observed(1), -1),
        ("weigh_observed", lambda: eng.weigh_observed(_abi.SCATTER_VARIANCE), -1),
        ("highpass_observed", lambda: eng.highpass_observed(), -1),
        ("normalise_observed", lambda: eng.normalise_observed(), -1),
    ]
    for name, call, code in refused:
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == code, (name, err.value)
        assert "trx_" + name in str(err.value), (name, err.value)
    assert (eng.nbands, eng.npix, eng.mom_shape) == (0, 0, (0, 0))
    again = eng.run(P.atm, P.opts)["spectrum"]
    assert np.array_equal(again, first)
    eng.close()
