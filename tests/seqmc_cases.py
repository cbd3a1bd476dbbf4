"""Shared SeqMC cases and reference helpers for test_seqmc_cpu.py / test_seqmc_gpu.py.

case(name) -> (targets, particles, seed): seeded, small (npart <= 1000 but for "npart-65537", steps <= 6, <= 4
targets but for "shape-ten-targets", regression n <= 48).  The runners oracle_run / library_run take such a triple
and return (samples [steps-burnin][d][npart], weights [steps-burnin][npart], flags [steps][ntargets]).

The exact_* helpers are references that share no code with orc_seqmc's reductions and search: the weights come
from the model's own log-density of the start particles, cp and var(W) from fractions.Fraction, the uniforms from
the Philox probe, and the resampling indices are read off the stored populations by value.
"""
import bisect
from fractions import Fraction

import numpy as np

import mcmchip as mc
import oracle_ref as orc
from mcmchip.seqmc import target_seed
from test_literal_reference import _block, _u52

README_NMOD = 10

# ------------------------------------------------------------------ samplers and targets
SAMPLERS = {
    "rwm": lambda: mc.RWM(0.5),
    "mala": lambda: mc.MALA(0.3),
    "mala_tuned": lambda: mc.MALA(0.3, mc.EmpMCTuner(0.6, adaptStep=1)),
    "hmc": lambda: mc.HMC(3, 0.2),
    "hmc_tuned": lambda: mc.HMC(2, 0.3, mc.EmpMCTuner(0.7, adaptStep=1, maxStep=5)),
    "hmcda": lambda: mc.HMCDA(len=2.0),             # its step stays 1 inside SeqMC: sigmas below stay > 0.5
    "ram": lambda: mc.RAM(0.5, 0.3),
    "block_rwm": lambda: mc.RWM(0.02),
    "block_mala": lambda: mc.MALA(0.005),
}
LAYOUT_DIMS = (1, 16, 24, 33, 70)      # lane per chain, its upper edge, two lanes per chain, wave per chain (x2)
LAYOUT_SAMPLERS = ("rwm", "mala_tuned", "hmc", "hmc_tuned", "hmcda")
SIGMAS = (3.0, 2.0, 1.5)               # tempered NormalDSL targets

TRIGGER = 0.05                         # var(W) < trigger both happens and does not over these runs (asserted)


def readme_targets(nmod, steps, burnin, trigger):
    """the first nmod of the README's ten tempered targets y = abs(x); y ~ Normal(1, s_i), RWM(s_i)"""
    sts = np.logspace(1, -1, README_NMOD)[:nmod]
    return [mc.model(mc.AbsNormalDSL(1.0, s), x=0.0) * mc.RWM(s) * mc.SeqMC(steps=steps, burnin=burnin, trigger=trigger)
            for s in sts]


def normal_targets(d, sname, steps, burnin, trigger, sigmas=SIGMAS, mu=0.0):
    r = mc.SeqMC(steps=steps, burnin=burnin, trigger=trigger)
    return [mc.model(mc.NormalDSL(mu, sg), v=np.zeros(d), gradient=True) * SAMPLERS[sname]() * r for sg in sigmas]


def regression_data(kind, n, d, xscale, seed):
    rng = np.random.default_rng(seed)
    X = xscale * rng.standard_normal((n, d))
    X[:, 0] = 1.0 * xscale
    eta = X @ rng.standard_normal(d)
    if kind == "logistic":
        return X, (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return X, eta + 0.5 * rng.standard_normal(n)


GLM_SAMPLERS = {"rwm": lambda: mc.RWM(0.05), "mala": lambda: mc.MALA(0.02), "hmcda": lambda: mc.HMCDA(len=2.0)}


def regression_targets(kind, n, d, sname, steps, burnin, trigger):
    """prior sigmas tempered across 3 targets; X scaled so that HMCDA's unit step inside SeqMC stays stable"""
    X, Y = regression_data(kind, n, d, 0.3 if d <= 8 else 0.1, 1000 + d)
    r = mc.SeqMC(steps=steps, burnin=burnin, trigger=trigger)
    out = []
    for ps in (4.0, 2.0, 1.0):
        t = mc.LogisticRegression(X, Y, prior_sigma=ps) if kind == "logistic" else mc.LinearRegression(X, Y, prior_sigma=ps)
        out.append(mc.model(t, vars=np.zeros(d), gradient=True) * GLM_SAMPLERS[sname]() * r)
    return out


def gamma_targets(steps, trigger, scale):
    """two Gamma targets on d = 1: particles below 0 are out of support (log-target -Inf)"""
    r = mc.SeqMC(steps=steps, burnin=0, trigger=trigger)
    return [mc.model(mc.DistDSL("Gamma", k, 1.0), v=np.array([1.0])) * mc.RWM(scale) * r for k in (2.0, 3.0)]


def _seed_of(name):
    return 1 + sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


def case(name):
    """(targets, particles [npart][d], seed) of a named case"""
    seed = _seed_of(name)
    rng = np.random.default_rng(seed)
    k = name.split("-")
    if k[0] == "layout":                                   # layout-d{d}-{sampler}
        d, sname = int(k[1][1:]), k[2]
        return normal_targets(d, sname, 5, 2, TRIGGER), 2.0 * rng.standard_normal((130, d)), seed
    if k[0] == "ram":                                      # ram-d{d}
        d = int(k[1][1:])
        return normal_targets(d, "ram", 5, 2, TRIGGER), 2.0 * rng.standard_normal((130, d)), seed
    if k[0] == "block":                                    # block-{rwm|mala}: d = 2049, block per chain
        # sigma near 1/sqrt(2 pi) keeps the 2049-term log-density, and so W = exp(.), away from underflow
        ts = normal_targets(2049, "block_" + k[1], 3, 1, TRIGGER, sigmas=(0.41, 0.40))
        return ts, 0.05 * rng.standard_normal((5, 2049)), seed
    if k[0] in ("logit", "linear"):                        # logit-d{3|130}-{sampler}[-p{npart}], linear-d5-mala
        d, sname = int(k[1][1:]), k[2]
        n = {3: 20, 130: 48, 5: 30}[d]
        npart = int(k[3][1:]) if len(k) > 3 else 70
        ts = regression_targets("logistic" if k[0] == "logit" else "linear", n, d, sname, 4, 1,
                                TRIGGER)
        return ts, 0.3 * rng.standard_normal((npart, d)), seed
    if k[0] == "npart":                                    # npart-{N}-{always|data}; npart-65537: chunk 257
        N = int(k[1])
        if N == 65537:
            return readme_targets(2, 2, 0, 0.05), rng.standard_normal((N, 1)), seed
        return readme_targets(4, 4, 0, 1e300 if k[2] == "always" else 0.05), rng.standard_normal((N, 1)), seed
    if name == "shape-steps1":
        return readme_targets(3, 1, 0, 0.05), rng.standard_normal((100, 1)), seed
    if name == "shape-burnin-last":                        # burnin = steps - 1: one stored row
        return readme_targets(3, 4, 3, 0.05), rng.standard_normal((100, 1)), seed
    if name == "shape-one-target":
        return readme_targets(1, 4, 1, 0.05), rng.standard_normal((100, 1)), seed
    if name == "shape-ten-targets":
        return readme_targets(10, 3, 0, 0.05), rng.standard_normal((100, 1)), seed
    if name == "python-default-particles":
        return normal_targets(1, "rwm", 3, 0, 0.05), None, seed
    raise KeyError(name)


# ------------------------------------------------------------------ runners
def oracle_run(targets, particles, seed):
    r = targets[-1].runner
    return orc.seqmc([(t.model, t.sampler) for t in targets], particles, r.steps, r.burnin, r.trigger, seed,
                     [target_seed(seed, k) for k in range(len(targets))])


def library_run(targets, particles, seed):
    ch = mc.run(targets, particles=particles, seed=seed)
    nst, _, npart = ch._samples.shape
    return ch._samples, ch.diagnostics["weigths"].reshape(nst, npart), ch.diagnostics["resampled"].astype(np.int32)


def bits_equal(a, b):
    """bitwise equality of two float64 arrays (NaNs compare by position and payload)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_run(got, want):
    s, w, f = got
    s0, w0, f0 = want
    assert np.array_equal(np.isnan(s), np.isnan(s0)) and np.array_equal(np.isnan(w), np.isnan(w0))
    assert np.array_equal(np.asarray(f, dtype=np.int32), np.asarray(f0, dtype=np.int32))
    assert bits_equal(s, s0)
    assert bits_equal(w, w0)


# ------------------------------------------------------------------ exact references (sections 2b, 2c)
def _one_normal_target(trigger):
    return [mc.model(mc.NormalDSL(0.0, 1.0), v=np.zeros(1)) * mc.RWM(0.5) * mc.SeqMC(steps=1, burnin=0, trigger=trigger)]


def exact_weights(model, particles):
    """W_n = exp(logW_n), logW_n = the model's log-target at the start particle (logtarget is zero before the first
    target, SeqMC.jl:60,70), as exact rationals of the doubles"""
    logW = orc.eval_batch(model, np.ascontiguousarray(np.asarray(particles, dtype=np.float64).T))[0]
    W = orc.detmath(1, logW)
    return W, [Fraction(float(v)) for v in W]


def exact_var(Wq):
    N = len(Wq)
    mean = sum(Wq) / N
    return sum((w - mean) ** 2 for w in Wq) / (N - 1)            # Julia var: N - 1


def exact_rs(Wq, seed, step=1, target=0):
    """(u_n, first p with cp_exact[p] >= u_n, in-band flag) per draw.  The computed cp[p] is two left-to-right sums
    of at most chunk + 256 positive terms and one division, so it lies within band = 2 (chunk + 257) 2^-53 cp[p]
    of cp_exact[p].  cp is nondecreasing, so only the two neighbours of u_n can hold it in their band."""
    N = len(Wq)
    total = sum(Wq)
    run, cp = Fraction(0), []
    for w in Wq:
        run += w
        cp.append(run / total)
    chunk = (N + 255) // 256
    eps = Fraction(2 * (chunk + 257), 2 ** 53)
    out = []
    for n in range(N):
        w = _block(seed, n, step, target, 2)
        u = Fraction(_u52(int(w[0]), int(w[1])))
        j = bisect.bisect_left(cp, u)
        near = (j < N and cp[j] - u <= eps * cp[j]) or (j > 0 and u - cp[j - 1] <= eps * cp[j - 1])
        out.append((u, j, near or not (0 < u < 1 - eps)))
    return out


def recover_rs(pop, row):
    """rs with row[n] == pop[rs[n]]: the mutated population's values are distinct"""
    assert len(np.unique(pop)) == len(pop)
    where = {float(v): p for p, v in enumerate(pop)}
    return np.array([where[float(v)] for v in row])


def mutate_and_resample(runner, targets_of, particles, seed):
    """the same one-step, one-target run never resampling (trigger 0) and always (1e300): the mutation does not
    depend on the trigger, so the second row is the first gathered by rs"""
    sA, wA, fA = runner(targets_of(0.0), particles, seed)
    sB, wB, fB = runner(targets_of(1e300), particles, seed)
    assert fA.shape == fB.shape == (1, 1) and fA[0, 0] == 0 and fB[0, 0] == 1
    return sA[0, 0], wA[0], recover_rs(sA[0, 0], sB[0, 0]), wB[0]


def check_exact_resampling(runner, particles, seed, zero=()):
    """section 2b (and 2c's flat runs) on `runner`: stored weights, rs, the weight reset and the trigger flag
    against exact rational arithmetic.  zero: indices whose weight must be exactly 0 and never selected."""
    P = np.asarray(particles, dtype=np.float64).reshape(-1, 1)
    N = len(P)
    model = _one_normal_target(0.0)[0].model
    W, Wq = exact_weights(model, P)
    pop, w_kept, rs, w_res = mutate_and_resample(runner, _one_normal_target, P, seed)
    assert bits_equal(w_kept, W)                                   # not resampled: exp(logW) of the start particle
    assert np.array_equal(w_res, np.ones(N))                       # resampled: logW = 0 (SeqMC.jl:85)
    assert sorted(np.flatnonzero(W == 0.0)) == sorted(zero)
    draws = exact_rs(Wq, seed)
    assert not any(near for _, _, near in draws), "a committed seed puts a draw into the rounding band"
    assert np.array_equal(rs, np.array([j for _, j, _ in draws]))
    assert not set(rs) & set(zero)
    # the flag is exact var(W, ddof=1) < trigger: a factor 2 on both sides, and (2N -+ 1) / 2N, between var and the
    # N-denominator's var (N-1)/N (resp. an (N-2)-denominator's); the computed var is ~N 2^-53 relative from exact
    v = exact_var(Wq)
    for num, den, want in ((2, 1, 1), (1, 2, 0), (2 * N + 1, 2 * N, 1), (2 * N - 1, 2 * N, 0)):
        trig = float(v * num / den)
        assert trig > 0.0 and np.isfinite(trig)
        _, _, f = runner(_one_normal_target(trig), P, seed)
        assert f[0, 0] == want, f"var(W) = {float(v):.17g}, trigger = {trig:.17g}"
    return rs


def exact_particles(N, seed):
    return np.random.default_rng(seed).standard_normal((N, 1))


EXACT_SIZES = (2, 7, 256, 257, 1000)          # 257: chunk 2, threads >= 129 own nothing
EXACT_SEED = {2: 21, 7: 22, 256: 23, 257: 24, 1000: 25}


def zero_block_particles(N, where, seed):
    """|x| >= 39 under Normal(0, 1): log-density < -760, W = exp(.) = 0 exactly; a block of N // 5 of them"""
    P = np.random.default_rng(seed).standard_normal((N, 1))
    nz = N // 5
    lo = {"head": 0, "middle": (N - nz) // 2, "tail": N - nz}[where]
    idx = np.arange(lo, lo + nz)
    P[idx, 0] = (39.0 + 0.01 * np.arange(nz)) * np.where(np.arange(nz) % 2 == 0, 1.0, -1.0)
    return P, list(idx)


ZERO_BLOCK_CASES = [(N, where) for N in (300, 64) for where in ("head", "middle", "tail")]


def check_all_zero_weights(runner):
    """every weight 0: total = 0, var = 0 < trigger, cp = 0/0 = NaN; `cp[mid] >= u` is false throughout, the search
    runs to its upper bound and every draw selects the last particle.  NaN arithmetic, not an error path."""
    N, seed = 50, 31
    P = (39.0 + 0.01 * np.arange(N)).reshape(N, 1)
    pop, w_kept, rs, w_res = mutate_and_resample(runner, _one_normal_target, P, seed)
    assert np.array_equal(w_kept, np.zeros(N)) and np.array_equal(w_res, np.ones(N))
    assert np.all(np.isfinite(pop))
    assert np.all((rs >= 0) & (rs < N))
    assert np.array_equal(rs, np.full(N, N - 1))


def check_single_particle(runner):
    """npart = 1: var(W) = 0/0 = NaN, `NaN < trigger` is false, so the runner never resamples and the weight stays
    exp(logW)"""
    ts = normal_targets(1, "rwm", 3, 0, 1e300, sigmas=SIGMAS[:2])
    s, w, f = runner(ts, np.array([[0.7]]), 41)
    assert not f.any()
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(w)) and np.all(w > 0.0)
    assert len(np.unique(w)) == 3                                  # logW keeps accumulating: never reset


GAMMA_BELOW = (3, 17, 18, 40, 59)


def gamma_particles(far):
    P = 0.5 + np.abs(np.random.default_rng(51).standard_normal((60, 1)))
    P[list(GAMMA_BELOW), 0] = -5.0 - np.arange(len(GAMMA_BELOW)) if far else -0.2 - 0.1 * np.arange(len(GAMMA_BELOW))
    return P


def check_gamma_always(runner):
    """out-of-support particles (logW = -Inf, W = 0) never survive the first resample, whether or not their
    mutation moved them into the support"""
    P, seed = gamma_particles(far=False), 52
    one = lambda trig: gamma_targets(1, trig, 0.5)[:1]
    pop, w_kept, rs, w_res = mutate_and_resample(runner, one, P, seed)
    assert np.array_equal(np.flatnonzero(w_kept == 0.0), np.array(GAMMA_BELOW))
    assert (pop[list(GAMMA_BELOW)] > 0).any()                      # some did move into the support
    assert not set(rs) & set(GAMMA_BELOW)
    s, w, f = runner(gamma_targets(3, 1e300, 0.5), P, seed)
    assert f.all() and np.array_equal(w, np.ones_like(w))
    assert np.all(np.isfinite(s)) and np.all(s > 0.0)


def check_gamma_never(runner):
    """trigger 0, particles far below 0 under a small RWM scale: every proposal stays out of support (ratio
    -Inf - -Inf = NaN, rejected), so logW = -Inf after the first target and -Inf + (-Inf - -Inf) = NaN after the
    second; the stored weights are NaN for exactly those particles"""
    P, seed = gamma_particles(far=True), 53
    s, w, f = runner(gamma_targets(3, 0.0, 0.1), P, seed)
    assert not f.any()
    bad = np.zeros(60, dtype=bool)
    bad[list(GAMMA_BELOW)] = True
    assert np.array_equal(np.isnan(w), np.broadcast_to(bad, w.shape))
    assert np.all(np.isfinite(w[:, ~bad])) and np.all(w[:, ~bad] > 0.0)
    assert np.all(np.isfinite(s)) and np.all(s[:, 0, bad] < 0.0) and np.all(s[:, 0, ~bad] > 0.0)


TIE_SEED = 102
TIE_PARTICLES = (float.fromhex("0x1.5dab1b54f8995p-1"), float.fromhex("0x1.3333333333333p-2"))


def check_tie_rule(runner):
    """findfirst(p -> p >= l, cp) (SeqMC.jl:82) at equality.  Two particles, crafted so that the computed
    cp[0] = W0 / (W0 + W1) -- at N = 2 the only association there is, the reference's cumsum(W) / sum(W) in IEEE
    doubles -- equals particle 0's uniform bit for bit: the draw selects particle 0, where `>` would select 1."""
    P = np.array(TIE_PARTICLES).reshape(2, 1)
    W, _ = exact_weights(_one_normal_target(0.0)[0].model, P)
    w = _block(TIE_SEED, 0, 1, 0, 2)
    u0 = _u52(int(w[0]), int(w[1]))
    cp = np.cumsum(W) / np.sum(W)
    assert cp[0] == u0 and cp[1] == 1.0                            # the precondition the particles were found for
    pop, w_kept, rs, w_res = mutate_and_resample(runner, _one_normal_target, P, TIE_SEED)
    assert bits_equal(w_kept, W)
    assert rs[0] == 0
