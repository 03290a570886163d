"""3DGS-MCMC density control without a GPU: the four entry points are exported and listed, and refuse NULL arguments before
anything touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C

NAMES = ("lcgs_mcmc_relocate", "lcgs_mcmc_add", "lcgs_mcmc_noise", "lcgs_mcmc_regularize")


def test_symbols_are_exported_and_listed(lcgs):
    lib = lcgs.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
    for method in ("mcmc_relocate", "mcmc_add", "mcmc_noise", "mcmc_regularize"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.mcmc_num_new)


def test_null_arguments_are_refused_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    pack = lcgs.api._Params(None, None, None, None, None)
    grads = lcgs.api._Grads(None, None, None, None, None)
    cfg = lcgs.api._McmcConfig(0.005, 51, 0)
    ncfg = lcgs.api._McmcNoiseConfig(5e5, 1.6e-4, 100.0, 0.995, 0, 1)
    n = C.c_int64(-1)
    p, c, nc, g = C.byref(pack), C.byref(cfg), C.byref(ncfg), C.byref(grads)
    fake_ctx = C.c_void_p(0)
    assert lib.lcgs_mcmc_relocate(fake_ctx, 4, 3, c, p, p, p, p, None, None, C.byref(n)) == 1  # LCGS_ERR_INVALID_ARG: NULL context
    assert b"NULL" in lib.lcgs_last_error()
    assert lib.lcgs_mcmc_add(fake_ctx, 4, 3, c, p, p, p, p, 2, 8, None, None) == 1
    assert lib.lcgs_mcmc_noise(fake_ctx, 4, nc, p, p, None) == 1
    assert lib.lcgs_mcmc_regularize(fake_ctx, 4, C.c_float(0.01), C.c_float(0.01), g) == 1
    # a NULL config / pack / count with a (never dereferenced) non-NULL context: refused by the first check too
    ctx = C.c_void_p(0x1000)
    assert lib.lcgs_mcmc_relocate(ctx, 4, 3, None, p, p, p, p, None, None, C.byref(n)) == 1
    assert lib.lcgs_mcmc_relocate(ctx, 4, 3, c, p, p, p, None, None, None, C.byref(n)) == 1
    assert lib.lcgs_mcmc_relocate(ctx, 4, 3, c, p, p, p, p, None, None, None) == 1
    assert lib.lcgs_mcmc_add(ctx, 4, 3, None, p, p, p, p, 2, 8, None, None) == 1
    assert lib.lcgs_mcmc_add(ctx, 4, 3, c, None, p, p, p, 2, 8, None, None) == 1
    assert lib.lcgs_mcmc_noise(ctx, 4, None, p, p, None) == 1
    assert lib.lcgs_mcmc_noise(ctx, 4, nc, p, None, None) == 1
    assert lib.lcgs_mcmc_regularize(ctx, 4, C.c_float(0.01), C.c_float(0.01), None) == 1
    # ... and so are an n_max outside 1..51 and a negative count, still before the context is read
    for bad in (0, 52):
        bad_cfg = lcgs.api._McmcConfig(0.005, bad, 0)
        assert lib.lcgs_mcmc_relocate(ctx, 4, 3, C.byref(bad_cfg), p, p, p, p, None, None, C.byref(n)) == 1
        assert b"n_max" in lib.lcgs_last_error()
    assert lib.lcgs_mcmc_add(ctx, 4, 3, c, p, p, p, p, -1, 8, None, None) == 1
    assert lib.lcgs_mcmc_noise(ctx, -1, nc, p, p, None) == 1
