"""What the tests of the metric-tensor samplers (SMMALA, PMALA, RMHMC, ERMLMC / RMLMC) share -- not collected.

A test file describes its sampler once as a Family; the device run is then held to the checker (manifold_ref) bit for
bit by Family.assert_same.  The rest are the helpers of the refusal and fork tests.
"""
import collections
import ctypes as ct
import functools
import os

import numpy as np
import pytest

import manifold_ref as mr
import mcmchip as mc
import smmala_cases as sc
from mcmchip import _lib

R40 = mc.SerialMC(steps=40, burnin=10, thinning=3)

# one checker run: kept samples, gradients and accept bits, the chains' final state by member, the evaluation count and
# (the trajectory samplers) the counters of what the steps covered
Ref = collections.namedtuple("Ref", "s g a state evals counters")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Family:
    """chains: the checker's Chains class; cases: the module of SHAPES and model(name); sampler(name, *key): the
    sampler a shape runs; manifold: the (device, checker) names of the mcmc_chains_manifold_state members held bit for
    bit beside x and lp; kernel: a text every step_kernel of the family carries"""

    def __init__(self, chains, cases, sampler, manifold=(), kernel=""):
        self.chains, self.cases, self.sampler, self.manifold, self.kernel = chains, cases, sampler, manifold, kernel
        self.keys = ("x", "lp") + tuple(ref for _, ref in manifold)
        self.reference = functools.lru_cache(maxsize=None)(self._reference)

    def _reference(self, name, *key):
        """the checker's R40 run of a shape, computed once, shared and read-only"""
        oc = self.chains(self.cases.model(name), self.sampler(name, *key), self.cases.SHAPES[name][3], seed=1)
        s, g, a = oc.run(R40)
        state = {k: getattr(oc, k).copy() for k in self.keys}
        for v in (s, g, a, *state.values()):
            v.setflags(write=False)
        return Ref(s, g, a, state, oc.evals, oc.counters)

    def state_of(self, oc):
        return {k: getattr(oc, k) for k in self.keys}

    def ran(self, oc, runner):
        """oc.run(runner) as a Ref on oc's live state"""
        s, g, a = oc.run(runner)
        return Ref(s, g, a, self.state_of(oc), oc.evals, oc.counters)

    def assert_same(self, ch, task, ref, what=""):
        assert np.isfinite(ref.s).all() and np.isfinite(ref.g).all(), what + ": the checker's chains carry a NaN"
        assert_outputs(ch, ref, what)
        assert np.array_equal(bits(ch.final_x), bits(ref.state["x"])), what + ": final_x"
        assert np.array_equal(bits(ch.final_lp), bits(ref.state["lp"])), what + ": final_lp"
        if self.manifold:
            ms = task.manifold_state()
            for dev, name in self.manifold:
                assert np.array_equal(bits(ms[dev]), bits(ref.state[name])), what + ": final " + name
        assert task.evals == ref.evals, what + ": evals"
        assert self.kernel in task.step_kernel, task.step_kernel


def assert_outputs(ch, ref, what="", chains=slice(None)):
    """the kept samples, gradients and accept bits of a run against the checker's chains `chains`"""
    assert np.array_equal(bits(ch._samples), bits(ref.s[:, :, chains])), what + ": samples"
    assert np.array_equal(bits(ch._gradients), bits(ref.g[:, :, chains])), what + ": gradients"
    assert np.array_equal(ch.diagnostics["accept"].T, ref.a[:, chains].astype(bool)), what + ": accept bits"


def fork_run(task, first, count, steps, d):
    """fork chains [first, first + count) of the task and run the fork `steps` steps, all kept: -> samples"""
    h = ct.c_void_p()
    _lib.check(_lib.load().mcmc_chains_fork(task.handle(), first, count, ct.byref(h)))
    try:
        samples = np.empty((steps, d, count))
        out = _lib.Outputs()
        out.samples = samples.ctypes.data
        rc = _lib.RunnerCfg(0, 1, steps)
        _lib.check(_lib.load().mcmc_run_serialmc(h, ct.byref(rc), ct.byref(out)))
    finally:
        _lib.load().mcmc_chains_destroy(h)
    return samples


def fork_reset_set_state(fam, m, sp, stale=None):
    """one run; a fork of chains [16, 48) continues exactly those chains; set_state by the sampler's :reset hook (stale:
    the manifold_state member the hook leaves as it was, and the next step uses); reset restarts"""
    r = mc.SerialMC(steps=20)
    oc = fam.chains(m, sp, 70, seed=5)
    t = (m * sp * r).batch(70, seed=5)
    first = fam.ran(oc, r)
    fam.assert_same(mc.run(t), t, first, "first run")
    samples = fork_run(t, 16, 32, 20, 5)
    ref = fam.ran(oc, r)
    assert np.array_equal(bits(samples), bits(ref.s[:, :, 16:48])), "fork"
    fam.assert_same(mc.run(t), t, ref, "source after fork")
    x = np.random.default_rng(9).standard_normal((5, 70)) * 0.3
    if stale:
        was = getattr(oc, dict(fam.manifold)[stale]).copy()
    lp = mc.reset(t, x)
    assert np.array_equal(bits(lp), bits(oc.set_state(x)))
    if stale:
        assert np.array_equal(bits(t.manifold_state()[stale]), bits(was))
    fam.assert_same(mc.run(t), t, fam.ran(oc, r), "after set_state")
    t.reset()
    oc.reset()
    if stale:
        assert np.array_equal(bits(t.manifold_state()[stale]), bits(getattr(oc, dict(fam.manifold)[stale])))
    last = fam.ran(oc, r)
    fam.assert_same(mc.run(t), t, last, "after reset")
    assert np.array_equal(bits(last.s), bits(first.s))


def _raises(code, text, f):
    with pytest.raises(_lib.MCMCError) as e:
        f()
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


def _create(m, cfg, C=4, x0=None):
    """mcmc_chains_create of C chains with the sampler configuration cfg, destroyed at once"""
    h = ct.c_void_p()
    try:
        _lib.check(_lib.load().mcmc_chains_create(m._handle(0), ct.byref(cfg), C, 0, ct.c_uint64(1),
                                                  None if x0 is None else _lib.dptr(x0), ct.byref(h)))
    finally:
        if h.value:
            _lib.load().mcmc_chains_destroy(h)


def gradient_refusals(nm, cfg, wide_text, dtensor=True):
    """mcmc_chains_create refuses d > 16 (wide_text) and a model with has_gradient 2 (for a sampler that needs dtensor),
    1 and 0, in the reference's words; -> the d = 17 model"""
    X, Y = sc.data(20, 17, 1)
    wide = mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(17), gradient=True, tensor=True, dtensor=dtensor)
    _raises(_lib.MCMC_E_UNSUPPORTED, wide_text, lambda: _create(wide, cfg))
    name = "logistic_n17_d5"
    if dtensor:
        _raises(_lib.MCMC_E_NEEDS_GRADIENT, nm + " sampler requires model with function of tensor derivatives",
                lambda: _create(sc.model(name), cfg))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, nm + " sampler requires model with tensor function",
            lambda: _create(sc.model(name, False), cfg))
    nograd = mc.model(sc.model(name).target, vars=np.zeros(5))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, nm + " sampler requires model with gradient function",
            lambda: _create(nograd, cfg))
    return wide


def store_leaps_refuses(task, name):
    buf = np.zeros(8 * 5 * 8)
    nl = np.zeros(8, dtype=np.int32)
    rc = _lib.load().mcmc_chains_store_leaps(task.handle(), 1, _lib.dptr(buf), _lib.dptr(buf), _lib.dptr(buf),
                                             _lib.dptr(buf), _lib.dptr(buf), nl.ctypes.data)
    assert rc == _lib.MCMC_E_UNSUPPORTED and name.encode() in _lib.load().mcmc_last_error()


def seqmc_refuses(task, name):
    """SeqMC refuses a task of 8 chains, d = 5, of the sampler `name` as a target (the config packed by hand)"""
    targets = (ct.c_void_p * 1)(task.handle())
    cfgq = (ct.c_int64 * 2)(2, 0)
    trig = ct.c_double(0.1)
    buf = (ct.c_char * 24)()
    ct.memmove(buf, cfgq, 16)
    ct.memmove(ct.addressof(buf) + 16, ct.addressof(trig), 8)
    parts = np.zeros((5, 8))
    rc = _lib.load().mcmc_run_seqmc(targets, 1, 8, parts.ctypes.data, ct.addressof(buf), ct.c_uint64(1), 0, None, None,
                                    None, None)
    assert rc == _lib.MCMC_E_UNSUPPORTED and name.encode() in _lib.load().mcmc_last_error()


def posterior_z(a, b, C):
    """per coordinate |difference of the grand means| over its standard error, the errors from the between-chain
    variance of the chain means of two runs of C independent chains each (samples [nkept][d][C])"""
    ca, cb = a.mean(axis=0), b.mean(axis=0)                          # chain means [d][C]
    ma, mb = ca.mean(axis=1), cb.mean(axis=1)
    se = np.sqrt(ca.var(axis=1, ddof=1) / C + cb.var(axis=1, ddof=1) / C)
    return np.abs(ma - mb) / se, ma, mb, se


def run_all(oc, r):
    """every step of a run with a burnin, kept: the tuner sees r.burnin, the kept range is the whole run"""
    oc.tuner_burnin = r.burnin
    return oc.run(mc.SerialMC(steps=r.len, burnin=0), nthreads=1)


def slabs(dGp, c, d):
    """dG [d, d, d] of point c from the checker's packed slabs [d, nr, C], slab r at [:, :, r]"""
    return np.stack([mr.unpack(dGp[r, :, c:c + 1], d)[:, :, 0] for r in range(d)], axis=2)


def python_refusals(nm, make, dtensor=True):
    """the constructor chain model * sampler * runner asks for the gradient, the tensor and (dtensor) the tensor's
    derivatives, in that order, without a device"""
    r = mc.SerialMC(steps=10)
    if dtensor:
        with pytest.raises(AssertionError, match=nm + " sampler requires model with function of tensor derivatives"):
            sc.model("probit_vaso") * make() * r
    with pytest.raises(AssertionError, match=nm + " sampler requires model with tensor function"):
        sc.model("probit_vaso", False) * make() * r
    nograd = mc.model(sc.model("probit_vaso").target, vars=np.zeros(3))
    with pytest.raises(AssertionError, match=nm + " sampler requires model with gradient function"):
        nograd * make() * r


def julia_texts():
    """the Julia hook's and module's source texts"""
    julia = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc.jl_amd", "julia")
    return tuple(open(os.path.join(julia, f)).read() for f in ("mcmc_jl_hook.jl", "MCMCHip.jl"))
