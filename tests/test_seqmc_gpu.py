"""SeqMC on the device: every state layout, sampler, population size, runner shape, weight edge and C ABI mode
mcmc_run_seqmc accepts, bitwise against the oracle's run_seqmc (samples, weights and flags as uint64 / int32
views, NaNs by position), plus the exact-rational and weight-edge checks of test_seqmc_cpu.py on the library."""
import ctypes as ct

import numpy as np
import pytest

import mcmchip as mc
import seqmc_cases as sc
from mcmchip import _lib
from mcmchip.seqmc import target_seed


def _parity(name, mixed=False):
    targets, particles, seed = sc.case(name)
    got = sc.library_run(targets, particles, seed)
    want = sc.oracle_run(targets, particles, seed)
    sc.assert_same_run(got, want)
    if mixed:
        f = want[2]
        assert 0 < f.sum() < f.size, f"{name}: flags {f.ravel()}"
    return got


# ------------------------------------------------------------------ layouts x samplers
@pytest.mark.gpu
@pytest.mark.parametrize("sname", sc.LAYOUT_SAMPLERS)
@pytest.mark.parametrize("d", sc.LAYOUT_DIMS)
def test_seqmc_layouts_and_samplers(gpu, d, sname):
    """lane per chain (1, 16), two lanes per chain (24), wave per chain (33, 70): cols_to_state, the reset eval,
    one step, state_to_cols.  Tuners keep their configured step, HMCDA its unit step."""
    _parity(f"layout-d{d}-{sname}", mixed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 28])
def test_seqmc_ram_targets(gpu, d):
    """RAM's jump factor adapts per particle slot across resets and resamples"""
    _parity(f"ram-d{d}", mixed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sname", ["rwm", "mala"])
def test_seqmc_block_per_chain(gpu, sname):
    """d = 2049: one block of four waves per particle"""
    _parity(f"block-{sname}", mixed=True)


# ------------------------------------------------------------------ regression targets
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logit-d3-rwm", "logit-d3-mala", "logit-d130-rwm", "logit-d130-mala",
                                  "logit-d3-hmcda-p40", "logit-d130-hmcda-p40", "linear-d5-mala"])
def test_seqmc_regression_targets(gpu, name):
    """the regression layout, d-sliced at d = 130; HMCDA with 40 > 16 particles runs its trajectories in identity
    chain order inside SeqMC (step_once sets no order), which changes no value: the oracle has no order at all"""
    _parity(name, mixed=True)


# ------------------------------------------------------------------ npart edges of the 256-chunk scan
@pytest.mark.gpu
@pytest.mark.parametrize("trig", ["always", "data"])
@pytest.mark.parametrize("npart", [1, 2, 63, 64, 65, 255, 256, 257, 511, 513])
def test_seqmc_npart_edges(gpu, npart, trig):
    s, w, f = _parity(f"npart-{npart}-{trig}")
    if trig == "always":
        assert f.all() == (npart > 1)                   # one particle: var = 0/0, never resampled


@pytest.mark.gpu
def test_seqmc_chunk_257(gpu):
    """65 537 particles: chunk 257, the last thread owns one particle"""
    _parity("npart-65537")


# ------------------------------------------------------------------ runner shapes
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shape-steps1", "shape-burnin-last", "shape-one-target", "shape-ten-targets"])
def test_seqmc_runner_shapes(gpu, name):
    s, w, f = _parity(name)
    targets = sc.case(name)[0]
    r = targets[-1].runner
    assert s.shape[0] == r.steps - r.burnin and f.shape == (r.steps, len(targets))


# ------------------------------------------------------------------ exact rationals and weight edges on the library
@pytest.mark.gpu
@pytest.mark.parametrize("npart", sc.EXACT_SIZES)
def test_seqmc_resampling_against_exact_rationals(gpu, npart):
    sc.check_exact_resampling(sc.library_run, sc.exact_particles(npart, sc.EXACT_SEED[npart]), sc.EXACT_SEED[npart])


@pytest.mark.gpu
def test_seqmc_draw_equal_to_cp_selects_that_particle(gpu):
    sc.check_tie_rule(sc.library_run)


@pytest.mark.gpu
@pytest.mark.parametrize("npart,where", sc.ZERO_BLOCK_CASES)
def test_seqmc_zero_weight_blocks_are_never_selected(gpu, npart, where):
    P, zero = sc.zero_block_particles(npart, where, 60 + npart)
    sc.check_exact_resampling(sc.library_run, P, 60 + npart, zero=zero)


@pytest.mark.gpu
def test_seqmc_all_zero_weights_select_the_last_particle(gpu):
    """cp is NaN throughout: the search is bounded by hi = N - 1 alone"""
    sc.check_all_zero_weights(sc.library_run)


@pytest.mark.gpu
def test_seqmc_single_particle_never_resamples(gpu):
    sc.check_single_particle(sc.library_run)


@pytest.mark.gpu
def test_seqmc_out_of_support_particles(gpu):
    sc.check_gamma_always(sc.library_run)
    sc.check_gamma_never(sc.library_run)
    for trig, scale, far in ((1e300, 0.5, False), (0.0, 0.1, True)):
        ts, P = sc.gamma_targets(3, trig, scale), sc.gamma_particles(far)
        sc.assert_same_run(sc.library_run(ts, P, 54), sc.oracle_run(ts, P, 54))


# ------------------------------------------------------------------ the C ABI's other modes
ABI_NPART, ABI_D, ABI_SEED = 50, 3, 77


def _abi_targets(steps=4, burnin=1):
    return sc.normal_targets(ABI_D, "mala", steps, burnin, sc.TRIGGER)


def _abi_call(targets, npart, particles, on_device, samples, weights, resampled, runtime, cfg=None, nchains=None):
    """mcmc_run_seqmc on fresh chain batches; pointers are integers (host or device addresses) or None"""
    batches = [mc.MCMCTask(t.model, t.sampler, t.runner, nchains=nchains or npart, seed=target_seed(ABI_SEED, k))
               for k, t in enumerate(targets)]
    handles = (ct.c_void_p * len(batches))(*[b.handle() for b in batches])
    cfg = cfg or targets[-1].runner.cfg()
    return _lib.load().mcmc_run_seqmc(handles, len(batches), npart, particles, ct.byref(cfg),
                                      ct.c_uint64(ABI_SEED), on_device, samples, weights, resampled, runtime)


@pytest.fixture(scope="module")
def abi_ref():
    targets = _abi_targets()
    P = 2.0 * np.random.default_rng(ABI_SEED).standard_normal((ABI_NPART, ABI_D))
    s, w, f = sc.oracle_run(targets, P, ABI_SEED)
    return np.ascontiguousarray(P.T), s, w, f


@pytest.mark.gpu
def test_seqmc_c_abi_on_device(gpu, abi_ref):
    import torch
    part, s0, w0, f0 = abi_ref
    dev = torch.device("cuda", 0)
    tp = torch.from_numpy(part).to(dev)
    ts = torch.full(s0.shape, -7.0, dtype=torch.float64, device=dev)
    tw = torch.full(w0.shape, -7.0, dtype=torch.float64, device=dev)
    tf = torch.full(f0.shape, -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rt = ct.c_double(-1.0)
    _lib.check(_abi_call(_abi_targets(), ABI_NPART, tp.data_ptr(), 1, ts.data_ptr(), tw.data_ptr(), tf.data_ptr(),
                         ct.byref(rt)))
    torch.cuda.synchronize()
    sc.assert_same_run((ts.cpu().numpy(), tw.cpu().numpy(), tf.cpu().numpy()), (s0, w0, f0))
    s, w, f = np.empty_like(s0), np.empty_like(w0), np.empty_like(f0)          # the host path, same call
    _lib.check(_abi_call(_abi_targets(), ABI_NPART, part.ctypes.data, 0, s.ctypes.data, w.ctypes.data, f.ctypes.data,
                         None))
    sc.assert_same_run((ts.cpu().numpy(), tw.cpu().numpy(), tf.cpu().numpy()), (s, w, f))
    assert np.array_equal(tp.cpu().numpy(), part) and rt.value > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("null", ["samples", "weights", "resampled", "runtime_s", "samples+weights"])
def test_seqmc_c_abi_null_outputs(gpu, abi_ref, null):
    """each output is optional; the others do not change (with samples NULL the store kernel writes to scratch)"""
    part, s0, w0, f0 = abi_ref
    s, w, f = np.full(s0.shape, -7.0), np.full(w0.shape, -7.0), np.full(f0.shape, -7, dtype=np.int32)
    rt = ct.c_double(-1.0)
    off = null.split("+")
    _lib.check(_abi_call(_abi_targets(), ABI_NPART, part.ctypes.data, 0,
                         None if "samples" in off else s.ctypes.data, None if "weights" in off else w.ctypes.data,
                         None if "resampled" in off else f.ctypes.data, None if "runtime_s" in off else ct.byref(rt)))
    for name, got, want in (("samples", s, s0), ("weights", w, w0)):
        assert np.all(got == -7.0) if name in off else sc.bits_equal(got, want)
    assert np.all(f == -7) if "resampled" in off else np.array_equal(f, f0)
    assert rt.value == -1.0 if "runtime_s" in off else rt.value > 0.0


@pytest.mark.gpu
def test_seqmc_c_abi_refusals(gpu, abi_ref):
    part, s0, w0, f0 = abi_ref
    s, w, f = np.empty_like(s0), np.empty_like(w0), np.empty_like(f0)
    args = (s.ctypes.data, w.ctypes.data, f.ctypes.data, None)
    with pytest.raises(mc.MCMCError, match="every target needs nchains == npart"):
        _lib.check(_abi_call(_abi_targets(), ABI_NPART, part.ctypes.data, 0, *args, nchains=ABI_NPART + 1))
    with pytest.raises(mc.MCMCError, match=r"Steps \(2\) should be > to burnin \(2\)"):
        cfg = _abi_targets()[-1].runner.cfg()
        cfg.steps, cfg.burnin = 2, 2
        _lib.check(_abi_call(_abi_targets(), ABI_NPART, part.ctypes.data, 0, *args, cfg=cfg))
    mixed = _abi_targets()[:2] + sc.normal_targets(ABI_D + 1, "mala", 4, 1, 0.05)[:1]
    with pytest.raises(mc.MCMCError, match="Models do not have the same parameter vector size"):
        _lib.check(_abi_call(mixed, ABI_NPART, part.ctypes.data, 0, *args))
    with pytest.raises(AssertionError, match="Models do not have the same parameter vector size"):
        mc.run(mixed, particles=part.T, seed=ABI_SEED)
    # a refused call leaves the library usable
    _lib.check(_abi_call(_abi_targets(), ABI_NPART, part.ctypes.data, 0, *args))
    sc.assert_same_run((s, w, f), (s0, w0, f0))


# ------------------------------------------------------------------ the Python surface
@pytest.mark.gpu
def test_resume_seqmc_is_a_fresh_run(gpu):
    """resume_seqmc (SeqMC.jl:125-128): the same targets under SeqMC(steps, trigger), burnin 0"""
    targets = _abi_targets(steps=4, burnin=1)
    trig = targets[-1].runner.trigger
    P = np.random.default_rng(5).standard_normal((40, ABI_D))
    ch = mc.resume_seqmc(targets, steps=3, particles=P, seed=9)
    fresh = [t.model * t.sampler * mc.SeqMC(steps=3, trigger=trig) for t in targets]
    want = sc.oracle_run(fresh, P, 9)
    assert ch._samples.shape == (3, ABI_D, 40)
    sc.assert_same_run((ch._samples, ch.diagnostics["weigths"].reshape(3, 40), ch.diagnostics["resampled"]), want)
    sc.assert_same_run(sc.library_run(fresh, P, 9), want)


@pytest.mark.gpu
def test_seqmc_default_particles(gpu):
    """particles=None: 100 standard normals per coordinate from numpy's Philox generator keyed by the seed"""
    targets, _, seed = sc.case("python-default-particles")
    ch = mc.run(targets, seed=seed)
    P = np.random.Generator(np.random.Philox(key=seed)).standard_normal((100, 1))
    assert ch._samples.shape == (3, 1, 100)
    sc.assert_same_run((ch._samples, ch.diagnostics["weigths"].reshape(3, 100), ch.diagnostics["resampled"]),
                       sc.oracle_run(targets, P, seed))
