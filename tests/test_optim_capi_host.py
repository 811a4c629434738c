"""CPU tests: argument rejections of nbp_adam_apply / nbp_sgd_apply (include/nbp.h).  Every call here is refused by
the entry's checks before anything is launched; the pointers are made-up addresses that are never dereferenced."""
import pytest

from lowlight_image_enhancement_amd import _lib

P, G, M, V, X, ST, CTL = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000  # 16-byte aligned
NBP_ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    return _lib.lib().dll


def _rejected(L, rc, text):
    assert rc == NBP_ERR_ARG
    assert text.encode() in L.nbp_last_error_string(), L.nbp_last_error_string()


def test_entries_are_declared_and_exported(L):
    sigs = _lib.parse_header()
    assert sigs["nbp_adam_apply"] == ("int", ["ptr"] * 5 + ["long", "ptr"] + ["double"] * 4 + ["int", "nbp_stream_t"])
    assert sigs["nbp_sgd_apply"] == ("int", ["ptr"] * 3 + ["long", "ptr", "ptr"] + ["double"] * 3 +
                                     ["int", "nbp_stream_t"])
    assert hasattr(L, "nbp_adam_apply") and hasattr(L, "nbp_sgd_apply")
    # nbp_optim_prepare and nbp_adamw_apply keep their signatures
    assert sigs["nbp_optim_prepare"] == ("int", ["ptr", "long", "float", "float", "ptr", "ptr", "float", "float",
                                                 "ptr", "ptr", "ptr", "ptr", "ptr", "int", "nbp_stream_t"])
    assert sigs["nbp_adamw_apply"] == ("int", ["ptr"] * 4 + ["long", "ptr"] + ["float"] * 4 + ["nbp_stream_t"])


def test_adam_apply_rejects_bad_arguments(L):
    hp = (0.9, 0.999, 1e-8, 0.01)
    good = [P, G, M, V, None, 1024, ST]
    for idx in (0, 1, 2, 3, 6):  # param, grad, exp_avg, exp_avg_sq, state: required
        a = list(good)
        a[idx] = None
        _rejected(L, L.nbp_adam_apply(*a, *hp, 0, None), "nbp_adam_apply: bad args")
    for n in (0, -4):
        a = list(good)
        a[5] = n
        _rejected(L, L.nbp_adam_apply(*a, *hp, 1, None), "nbp_adam_apply: bad args")
    for idx in (0, 1, 2, 3, 4):  # every stream moves in 16-byte words (max_exp_avg_sq too when given)
        for off in (4, 8, 12):
            a = list(good)
            a[idx] = (a[idx] or X) + off
            _rejected(L, L.nbp_adam_apply(*a, *hp, 1, None), "nbp_adam_apply: buffers must be 16-byte aligned")


def test_sgd_apply_rejects_bad_arguments(L):
    good = [P, G, M, 1024, ST, CTL]
    for idx in (0, 1, 4, 5):  # param, grad, state, ctl: required
        a = list(good)
        a[idx] = None
        _rejected(L, L.nbp_sgd_apply(*a, 0.9, 0.0, 0.0, 0, None), "nbp_sgd_apply: bad args")
    for n in (0, -1):
        a = list(good)
        a[3] = n
        _rejected(L, L.nbp_sgd_apply(*a, 0.9, 0.0, 0.0, 0, None), "nbp_sgd_apply: bad args")
    # the momentum buffer is null exactly when momentum == 0
    _rejected(L, L.nbp_sgd_apply(P, G, None, 1024, ST, CTL, 0.9, 0.0, 0.0, 0, None), "momentum_buf is needed exactly")
    _rejected(L, L.nbp_sgd_apply(P, G, M, 1024, ST, CTL, 0.0, 0.0, 0.0, 0, None), "momentum_buf is needed exactly")
    # torch: "Nesterov momentum requires a momentum and zero dampening"
    _rejected(L, L.nbp_sgd_apply(P, G, None, 1024, ST, CTL, 0.0, 0.0, 0.0, 1, None), "nesterov requires")
    _rejected(L, L.nbp_sgd_apply(P, G, M, 1024, ST, CTL, -0.5, 0.0, 0.0, 1, None), "nesterov requires")
    _rejected(L, L.nbp_sgd_apply(P, G, M, 1024, ST, CTL, 0.9, 0.1, 0.0, 1, None), "nesterov requires")
    for idx in (0, 1, 2):
        for off in (4, 8, 12):
            a = list(good)
            a[idx] += off
            _rejected(L, L.nbp_sgd_apply(*a, 0.9, 0.0, 0.0, 0, None), "nbp_sgd_apply: buffers must be 16-byte aligned")
