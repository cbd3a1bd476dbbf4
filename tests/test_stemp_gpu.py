"""SerialTempMC on the device, bitwise against the checker (tests/stemp_oracle.c): samples, the `mod` rows, the swap
bits, the final `at`, and every target's step counter, evaluation count and state.  tests/test_stemp_cpu.py holds the
checker against a literal transcription of run_serialtempmc and shows that every case of the table accepts and rejects
swaps and visits every target, where its logW allows."""
import ctypes as ct

import numpy as np
import pytest

import mcmchip as mc
import smmala_cases as smc
import stemp_cases as sc
from mcmchip import _lib
from mcmchip.seqmc import target_seed


def _parity(run, on_device=0):
    got, batches = sc.library_run(run, on_device=on_device)
    want, chains = sc.oracle_run(run)
    sc.assert_same_run(got, want)
    sc.check_expectation(run.cs, want["counters"], run.C)
    sc.assert_same_targets(batches, chains)
    return got


# ------------------------------------------------------------------ layouts, samplers, K, C, swapPeriod, burnin, logW
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_stemp_parity(gpu, name):
    _parity(sc.Run(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iso-rwm-k3-c65-p2", "wave-mala-k3-c65-p2", "logit-mala-k3-c64-p2"])
def test_stemp_on_device_outputs(gpu, name):
    """device pointers for samples, models, swap_bits and final_at: the same run as with host buffers"""
    _parity(sc.Run(name), on_device=1)


@pytest.mark.gpu
@pytest.mark.parametrize("null", ["samples", "models", "swap_bits", "final_at", "runtime_s", "all"])
def test_stemp_null_outputs(gpu, null):
    """each output is optional; the others do not change"""
    run = sc.Run("iso-rwm-k3-c65-p2")
    want, _ = sc.oracle_run(run)
    nst, C, d = want["samples"].shape[0], run.C, run.d
    s, m = np.full((nst, d, C), -7.0), np.full((nst, C), -7, dtype=np.int32)
    b, a = np.zeros((nst, 2), dtype=np.uint64), np.full(C, -7, dtype=np.int32)
    rt = ct.c_double(-1.0)
    off = ("samples", "models", "swap_bits", "final_at", "runtime_s") if null == "all" else (null,)
    ptr = lambda nm, arr: None if nm in off else arr.ctypes.data  # noqa: E731
    _lib.check(sc.abi_call(run.batches(), C, run.runner().cfg(), run.logW, run.seed, 0, ptr("samples", s),
                           ptr("models", m), ptr("swap_bits", b), ptr("final_at", a),
                           None if "runtime_s" in off else ct.byref(rt)))
    assert np.all(s == -7.0) if "samples" in off else sc.bits_equal(s, want["samples"])
    assert np.all(m == -7) if "models" in off else np.array_equal(m, want["mod"])
    assert np.all(a == -7) if "final_at" in off else np.array_equal(a, want["final_at"])
    bits = np.unpackbits(b.view(np.uint8).reshape(nst, -1), axis=1, bitorder="little")[:, :C].astype(bool)
    assert not bits.any() if "swap_bits" in off else np.array_equal(bits, want["swap"])
    assert rt.value == -1.0 if "runtime_s" in off else rt.value > 0.0


# ------------------------------------------------------------------ chain ids and counters
@pytest.mark.gpu
def test_stemp_split_batch(gpu):
    """walkers of batches created at chain offset 64 are the walkers with those global ids of a larger batch"""
    name = "iso-rwm-k3-c65-p2"
    whole, _ = sc.library_run(sc.Run(name, C=129))
    part_run = sc.Run(name, C=65, offset=64)
    part, _ = sc.library_run(part_run)
    assert sc.bits_equal(part["samples"], whole["samples"][:, :, 64:])
    assert np.array_equal(part["mod"], whole["mod"][:, 64:]) and np.array_equal(part["swap"], whole["swap"][:, 64:])
    assert np.array_equal(part["final_at"], whole["final_at"][64:])
    sc.assert_same_run(part, sc.oracle_run(part_run)[0])
    assert part["swap"].any() and not part["swap"].all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iso-mala-k2-c64-p5-b7", "iso-ram-k2-c64-p2"])
def test_stemp_second_run_continues_the_targets(gpu, name):
    """a second run on the same batches: every target's sampler draws go on from its step counter (and RAM's factors
    from where they stood); the walkers start again on target 0, from where its chains stand"""
    run = sc.Run(name)
    first, batches = sc.library_run(run)
    second, _ = sc.library_run(run, batches=batches)
    want1, chains = sc.oracle_run(run)
    want2, _ = sc.oracle_run(run, chains=chains)
    sc.assert_same_run(first, want1)
    sc.assert_same_run(second, want2)
    assert not sc.bits_equal(first["samples"], second["samples"])
    assert [b.steps_done for b in batches] == [2 * (run.cs["steps"] + 1)] + [2 * run.cs["steps"]] * (run.K - 1)
    sc.assert_same_targets(batches, chains)


# ------------------------------------------------------------------ refusals and errors
def _call(batches, C, steps=4):
    cfg = mc.SerialTempMC(steps=steps, swapPeriod=2).cfg()
    return sc.abi_call(batches, C, cfg, None, 5, 0, None, None, None, None, None)


def _refused(batches, C, code, text):
    rc = _call(batches, C)
    msg = _lib.load().mcmc_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


@pytest.mark.gpu
def test_stemp_refuses_nuts_and_smmala_targets(gpu):
    r = mc.SerialTempMC(steps=4)
    m = mc.model(mc.NormalDSL(0.0, 1.0), v=np.zeros(3), gradient=True)
    ok = mc.MCMCTask(m, mc.MALA(0.3), r, nchains=8)
    nuts = mc.MCMCTask(m, mc.NUTS(), r, nchains=8)
    _refused([ok, nuts], 8, _lib.MCMC_E_UNSUPPORTED,
             "SerialTempMC does not run NUTS targets: NUTS adapts epsilon by its own step counter (NUTS.jl:166)")
    g = smc.logistic_40_10()
    sm = [mc.MCMCTask(g, mc.SMMALA(0.5), r, nchains=8), mc.MCMCTask(g, mc.MALA(0.02), r, nchains=8)]
    _refused(sm, 8, _lib.MCMC_E_UNSUPPORTED,
             "SerialTempMC does not run SMMALA targets: the sampler's reset hook keeps invG and firstTerm")
    assert "SeqMC" not in _lib.load().mcmc_last_error().decode()
    with pytest.raises(mc.MCMCError, match="SerialTempMC does not run NUTS targets"):
        mc.run([m * mc.MALA(0.3) * r, m * mc.NUTS() * r], nwalkers=8)


@pytest.mark.gpu
def test_stemp_invalid_arguments(gpu):
    r = mc.SerialTempMC(steps=4)
    m3 = mc.model(mc.NormalDSL(0.0, 1.0), v=np.zeros(3))
    m4 = mc.model(mc.NormalDSL(0.0, 1.0), v=np.zeros(4))
    mk = lambda m, C=8, **kw: mc.MCMCTask(m, mc.RWM(0.5), r, nchains=C, **kw)  # noqa: E731
    E = _lib.MCMC_E_INVALID_ARG
    _refused([mk(m3)], 8, E, "at least two targets")                                         # K = 1
    _refused([mk(m3), mk(m4)], 8, E, "Models do not have the same parameter vector size")     # mixed d
    _refused([mk(m3), mk(m3)], 9, E, "every target needs nchains == nwalkers")                # nwalkers != C
    _refused([mk(m3), mk(m3, C=9)], 8, E, "every target needs nchains == nwalkers")
    _refused([mk(m3), mk(m3, chain_offset=64)], 8, E, "same chain offset")
    # a target on a second context of the same device
    lib = _lib.load()
    ctx2, mh, ch = ct.c_void_p(), ct.c_void_p(), ct.c_void_p()
    _lib.check(lib.mcmc_ctx_create(0, ct.byref(ctx2)))
    desc, cfg = m3._desc(), mc.RWM(0.5).cfg()
    _lib.check(lib.mcmc_model_create(ctx2, ct.byref(desc), ct.byref(mh)))
    _lib.check(lib.mcmc_chains_create(mh, ct.byref(cfg), 8, 0, ct.c_uint64(1), None, ct.byref(ch)))

    class _Foreign:
        def handle(self):
            return ch
    try:
        _refused([mk(m3), _Foreign()], 8, E, "targets live on different contexts")
    finally:
        _lib.check(lib.mcmc_chains_destroy(ch))
        _lib.check(lib.mcmc_model_destroy(mh))
        _lib.check(lib.mcmc_ctx_destroy(ctx2))
    bad = mc.SerialTempMC(steps=4).cfg()
    bad.swap_period = 0
    assert sc.abi_call([mk(m3), mk(m3)], 8, bad, None, 5, 0, None, None, None, None, None) == E
    # a refused call leaves the library usable
    assert _call([mk(m3), mk(m3)], 8) == 0


# ------------------------------------------------------------------ the Python surface
@pytest.mark.gpu
def test_stemp_python_api(gpu):
    """run([m1 * s * r, m2 * s * r], nwalkers, logW, seed): one MCMCChain with diagnostics mod and swap"""
    run = sc.Run("iso-rwm-k3-c65-p2")
    ch = mc.run(run.tasks(), nwalkers=run.C, seed=run.seed)
    assert isinstance(ch, mc.MCMCChain)
    nst = run.cs["steps"] - run.cs["burnin"]
    assert ch.samples.shape == (run.C, nst, run.d)
    assert ch.diagnostics["mod"].shape == (run.C, nst) and ch.diagnostics["swap"].shape == (run.C, nst)
    assert ch.diagnostics["swap"].dtype == bool and ch.range == range(1, run.cs["steps"] + 1) and ch.runTime > 0.0
    # the same walkers as the checker's from model.init (the tasks carry no per-walker start)
    import oracle_ref as orc
    import stemp_ref
    chains = [orc.OracleChains(m, s, nchains=run.C, seed=target_seed(run.seed, k))
              for k, (m, s) in enumerate(run.pairs)]
    want = stemp_ref.serialtempmc(chains, run.cs["steps"], run.cs["burnin"], run.cs["period"], None, run.seed)
    assert sc.bits_equal(ch._samples, want["samples"])
    assert np.array_equal(ch.diagnostics["mod"], want["mod"].T)
    assert np.array_equal(ch.diagnostics["swap"], want["swap"].T)
    assert np.array_equal(ch.diagnostics["final_mod"], want["final_at"])
    assert len(set(ch.diagnostics["mod"].ravel())) == run.K
    # logW reaches the library: the forced vector keeps every walker on task 0
    ts = sc.Run("iso-rwm-k2-c65-stay").tasks()
    stay = mc.run(ts, nwalkers=5, logW=[0.0, -800.0], seed=3)
    assert not stay.diagnostics["mod"].any() and not stay.diagnostics["swap"].any()
    # the reference's default: one walker
    one = mc.run(ts)
    assert one.samples.shape == (1, 12, 3)
    # resume_serialtempmc: new tasks under SerialTempMC(steps, swapPeriod), burnin 0
    res = mc.resume(ch, steps=6, seed=run.seed)
    assert res.samples.shape == (run.C, 6, run.d) and res.task[-1].runner.swapPeriod == run.cs["period"]
    fresh = [orc.OracleChains(m, s, nchains=run.C, seed=target_seed(run.seed, k)) for k, (m, s) in enumerate(run.pairs)]
    want = stemp_ref.serialtempmc(fresh, 6, 0, run.cs["period"], None, run.seed)
    assert sc.bits_equal(res._samples, want["samples"])
