"""The SerialTempMC case table and runners shared by test_stemp_cpu.py / test_stemp_gpu.py.

CASES[name] is a small seeded run: K targets of one layout and sampler, C walkers, steps <= 60.  `expect` says what
the swap counters must show (test_stemp_cpu.py checks it on the checker, so that every GPU parity case is known to
exercise what it is there for):
  mixed  swaps accepted and rejected, every target visited
  up     logW = (0, +800): the one swap 0 -> 1 of every walker is accepted, every swap back rejected
  stay   logW = (0, -800): no swap is ever accepted, target 1 never visited
  never  swapPeriod = steps + 1: no swap is proposed
"""
import ctypes as ct

import numpy as np

import mcmchip as mc
import oracle_ref as orc
import stemp_ref
from mcmchip import _lib
from mcmchip.seqmc import target_seed

SIGMAS = (3.0, 2.0, 1.5, 1.2, 1.0)          # tempered NormalDSL targets, widest first
WAVE_SIGMAS = (1.5, 1.45, 1.4, 1.35, 1.3)  # d = 40: d log(s1 / s2) has to stay of order one for swaps both ways
PRIORS = (2.0, 1.8, 1.6, 1.5, 1.4)          # tempered prior sigmas of the logistic targets (close: swaps both ways)

SAMPLERS = {
    "rwm": lambda: mc.RWM(0.5),
    "mala": lambda: mc.MALA(0.3),
    "hmc": lambda: mc.HMC(3, 0.2),
    "ram": lambda: mc.RAM(0.5, 0.3),
    "glm_rwm": lambda: mc.RWM(0.05),
    "glm_mala": lambda: mc.MALA(0.02),
    "glm_hmc": lambda: mc.HMC(3, 0.05),
}


def _c(layout, sampler, K, C, steps, burnin, period, logW=None, expect="mixed"):
    return dict(layout=layout, sampler=sampler, K=K, C=C, steps=steps, burnin=burnin, period=period, logW=logW,
                expect=expect)


FINITE = (0.0, 0.7, -0.4, 0.2, -1.1)

# layouts: iso (lane per chain, d = 3, target 0 the IsoNormalDot model), pair (two lanes per chain, d = 20), wave
# (wave per chain, d = 40), logit (the regression layout, logistic n = 40, d = 5)
CASES = {
    "iso-rwm-k3-c65-p2": _c("iso", "rwm", 3, 65, 40, 0, 2),
    "iso-mala-k2-c64-p5-b7": _c("iso", "mala", 2, 64, 40, 7, 5),
    "iso-hmc-k5-c63-p1-finite": _c("iso", "hmc", 5, 63, 30, 3, 1, FINITE),
    "iso-ram-k2-c64-p2": _c("iso", "ram", 2, 64, 30, 0, 2),
    "iso-rwm-k2-c1-p1": _c("iso", "rwm", 2, 1, 60, 0, 1),
    "iso-rwm-k5-c257-p1-finite": _c("iso", "rwm", 5, 257, 30, 1, 1, FINITE),
    "iso-rwm-k2-c65-up": _c("iso", "rwm", 2, 65, 12, 0, 2, (0.0, 800.0), "up"),
    "iso-rwm-k2-c65-stay": _c("iso", "rwm", 2, 65, 12, 0, 2, (0.0, -800.0), "stay"),
    "iso-mala-k3-c65-never": _c("iso", "mala", 3, 65, 10, 3, 11, None, "never"),
    "pair-rwm-k3-c65-p2": _c("pair", "rwm", 3, 65, 20, 3, 2),
    "pair-mala-k2-c64-p5": _c("pair", "mala", 2, 64, 30, 7, 5, FINITE[:2]),
    "pair-hmc-k3-c63-p2": _c("pair", "hmc", 3, 63, 16, 0, 2),
    "wave-rwm-k2-c257-p1": _c("wave", "rwm", 2, 257, 10, 0, 1),
    "wave-mala-k3-c65-p2": _c("wave", "mala", 3, 65, 14, 3, 2),
    "wave-hmc-k2-c63-p5": _c("wave", "hmc", 2, 63, 20, 7, 5),
    "logit-rwm-k5-c65-p1": _c("logit", "glm_rwm", 5, 65, 20, 0, 1),
    "logit-mala-k3-c64-p2": _c("logit", "glm_mala", 3, 64, 20, 3, 2, FINITE[:3]),
    "logit-hmc-k2-c63-p5": _c("logit", "glm_hmc", 2, 63, 20, 7, 5),
}
DIMS = {"iso": 3, "pair": 20, "wave": 40, "logit": 5}


def seed_of(name):
    return 1 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def _logit_data():
    rng = np.random.default_rng(4005)
    X = 0.3 * rng.standard_normal((40, 5))
    X[:, 0] = 0.3
    Y = (rng.random(40) < 1.0 / (1.0 + np.exp(-(X @ rng.standard_normal(5))))).astype(np.float64)
    return X, Y


def models_of(layout, K):
    d = DIMS[layout]
    if layout == "logit":
        X, Y = _logit_data()
        return [mc.model(mc.LogisticRegression(X, Y, prior_sigma=ps), vars=np.zeros(d), gradient=True)
                for ps in PRIORS[:K]]
    ms = [mc.model(mc.NormalDSL(0.0, sg), v=np.zeros(d), gradient=True) for sg in (WAVE_SIGMAS if layout == "wave" else SIGMAS)[:K]]
    if layout == "iso":
        ms[0] = mc.model(mc.IsoNormalDot(), init=np.zeros(d), grad=True)
    return ms


class Run:
    """The targets of a case as (model, sampler) pairs, the walkers' start [d][C] and the run's seed; `offset` the
    first walker's global chain id."""

    def __init__(self, name, C=None, offset=0, **over):
        cs = dict(CASES[name], **over)
        self.cs, self.name, self.offset = cs, name, offset
        self.K, self.C = cs["K"], cs["C"] if C is None else C
        self.d = DIMS[cs["layout"]]
        self.seed = seed_of(name)
        self.pairs = [(m, SAMPLERS[cs["sampler"]]()) for m in models_of(cs["layout"], self.K)]
        # a start per global chain id, so that a batch at an offset starts where the larger batch's walkers do
        scale = 0.3 if cs["layout"] == "logit" else 1.5
        allx = scale * np.random.default_rng(self.seed).standard_normal((self.d, 600))
        self.init_x = np.ascontiguousarray(allx[:, offset:offset + self.C])
        self.logW = None if cs["logW"] is None else np.array(cs["logW"], dtype=np.float64)

    def runner(self):
        return mc.SerialTempMC(steps=self.cs["steps"], burnin=self.cs["burnin"], swapPeriod=self.cs["period"])

    def tasks(self):
        r = self.runner()
        return [m * s * r for m, s in self.pairs]

    def oracle_chains(self):
        return [orc.OracleChains(m, s, nchains=self.C, seed=target_seed(self.seed, k), chain_offset=self.offset,
                                 init_x=self.init_x.copy()) for k, (m, s) in enumerate(self.pairs)]

    def batches(self):
        r = self.runner()
        return [mc.MCMCTask(m, s, r, nchains=self.C, seed=target_seed(self.seed, k), chain_offset=self.offset,
                            init_x=self.init_x) for k, (m, s) in enumerate(self.pairs)]


def oracle_run(run, chains=None):
    chains = run.oracle_chains() if chains is None else chains
    cs = run.cs
    return stemp_ref.serialtempmc(chains, cs["steps"], cs["burnin"], cs["period"], run.logW, run.seed), chains


def abi_call(batches, C, cfg, logW, seed, on_device, samples, models, bits, final_at, runtime):
    """mcmc_run_serialtempmc; pointers are integers (host or device addresses) or None"""
    handles = (ct.c_void_p * len(batches))(*[b.handle() for b in batches])
    return _lib.load().mcmc_run_serialtempmc(handles, len(batches), C, ct.byref(cfg),
                                             None if logW is None else logW.ctypes.data,
                                             ct.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), on_device, samples, models, bits,
                                             final_at, runtime)


def library_run(run, batches=None, on_device=0):
    """-> (dict like stemp_ref.serialtempmc's without counters, batches)"""
    batches = run.batches() if batches is None else batches
    cs, C, d = run.cs, run.C, run.d
    nst, nw = cs["steps"] - cs["burnin"], (C + 63) // 64
    cfg = run.runner().cfg()
    rt = ct.c_double(-1.0)
    if on_device:
        import torch
        dev = torch.device("cuda", 0)
        ts = torch.full((nst, d, C), -7.0, dtype=torch.float64, device=dev)
        tm = torch.full((nst, C), -7, dtype=torch.int32, device=dev)
        tb = torch.full((nst, nw), -7, dtype=torch.int64, device=dev)
        ta = torch.full((C,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        _lib.check(abi_call(batches, C, cfg, run.logW, run.seed, 1, ts.data_ptr(), tm.data_ptr(), tb.data_ptr(),
                            ta.data_ptr(), ct.byref(rt)))
        torch.cuda.synchronize()
        s, m, a = ts.cpu().numpy(), tm.cpu().numpy(), ta.cpu().numpy()
        b = tb.cpu().numpy().view(np.uint64)
    else:
        s, m = np.full((nst, d, C), -7.0), np.full((nst, C), -7, dtype=np.int32)
        b, a = np.zeros((nst, nw), dtype=np.uint64), np.full(C, -7, dtype=np.int32)
        _lib.check(abi_call(batches, C, cfg, run.logW, run.seed, 0, s.ctypes.data, m.ctypes.data, b.ctypes.data,
                            a.ctypes.data, ct.byref(rt)))
    assert rt.value > 0.0
    swap = np.unpackbits(np.ascontiguousarray(b).view(np.uint8).reshape(nst, -1), axis=1, bitorder="little")
    assert not swap[:, C:].any()                         # the bits past the last walker stay clear
    return {"samples": s, "mod": m, "swap": swap[:, :C].astype(bool), "final_at": a}, batches


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_run(got, want):
    assert np.array_equal(got["mod"], want["mod"])
    assert np.array_equal(got["swap"], want["swap"])
    assert np.array_equal(got["final_at"], want["final_at"])
    assert bits_equal(got["samples"], want["samples"])


def assert_same_targets(batches, chains):
    """every target's step counter, evaluation count and state: the state through one further SerialMC step of the
    batch and of its oracle twin (same position, log-target, RAM factor and counter <=> same step)"""
    one = mc.SerialMC(steps=1)
    for k, (b, oc) in enumerate(zip(batches, chains)):
        assert b.steps_done == oc.steps_done, f"target {k}: steps_done"
        assert b.evals == int(oc.n_evals.sum()), f"target {k}: evals"
        if oc.kind == 5:
            assert bits_equal(b.ram_factor(), mc.api.unpack_ram_factor(oc.ram_L, oc.om.size)), f"target {k}: RAM factor"
        b.runner = one
        ch = mc.run(b)
        s, _, acc = oc.run(one)
        assert bits_equal(ch._samples, s), f"target {k}: state"
        assert np.array_equal(ch.diagnostics["accept"].T, acc.astype(bool)), f"target {k}: accept"


def check_expectation(cs, cnt, C):
    """the case does what it is in the table for (counters of the checker)"""
    nswap = sum(1 for i in range(1, cs["steps"] + 1) if i % cs["period"] == 0)
    assert cnt["proposed"] == nswap * C and cnt["accepted"] + cnt["rejected"] == cnt["proposed"]
    assert sum(cnt["visits"]) == cs["steps"] * C
    if cs["expect"] == "mixed":
        assert cnt["accepted"] > 0 and cnt["rejected"] > 0
        assert all(v > 0 for v in cnt["visits"]), cnt["visits"]
    elif cs["expect"] == "up":
        assert cnt["accepted"] == C and cnt["rejected"] == (nswap - 1) * C and cnt["visits"][1] > cnt["visits"][0]
    elif cs["expect"] == "stay":
        assert cnt["accepted"] == 0 and cnt["visits"][1:] == [0] * (cs["K"] - 1)
    else:
        assert cnt["proposed"] == 0 and cnt["visits"][1:] == [0] * (cs["K"] - 1)
