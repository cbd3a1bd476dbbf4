"""Shared cases for the separable targets (IsoNormalDot, NormalDSL, AbsNormalDSL, DistDSL) on every step-kernel
instance their width can select: test_separable_cpu.py (CPU: the table names every instance, the oracle's run of
every case both accepts and rejects, the oracle against a high-precision sum) and test_separable_instances.py (GPU:
bitwise against the oracle).

The kernel families, restated here from the widths alone (not read from the library):
  d <= 16           lane per chain,      lpc_*<NB, F, M>, NB = ceil(d/4) Philox blocks a lane
  17 <= d <= 32     two lanes per chain, lpp_*<NBL, F, M>, NBL = ceil(NB/2): the first lane holds coordinates
                    0 .. 4 NBL - 1, the second the rest (fewer blocks when NB is odd)
  33 <= d <= 2048   wave per chain,      wpc_*<NB, F, M>, NB = 1, 2, 4, 8 slots of 256 coordinates
                    (lane l, slot k holds 4 (l + 64 k) .. + 3)
  2049 <= d <= 16384 block per chain,    bpc_*<W, M>, W = 4, 8 waves, 8 slots of 256 W coordinates
F (every lane coordinate is a real one) is built for IsoDot and NormalDSL lane / pair kernels and for IsoDot wave
kernels.  RWM on few chains (C <= 64) takes the look-ahead kernels instead; the cases keep C above that.

No RNG in the table: inits, scales and step sizes are closed forms of d.
"""
from collections import namedtuple

import numpy as np

import mcmchip as mc

MODELS = ("IsoDot", "NormalDSL", "AbsNormalDSL", "DistDSL")
KINDS = ("rwm", "mala", "hmc", "hmcda")
LA_MAX_CHAINS = 64                       # RWM at C <= 64 runs lpc_rwm_la (one chain: lpc_rwm_spec for d <= 4)
FULL_LANE = ("IsoDot", "NormalDSL")      # models whose lane / pair kernels have the F instances
FULL_WAVE = ("IsoDot",)
D_MAX = 16384

# both sides of every class edge and a width off the 4-coordinate grid inside every class; 3 as well, because d = 1
# has one scale (always uniform) and d = 4 is the F instance: lpc_rwm<1, false, M, false> needs d = 2 or 3
D_SWEEP = (1, 3, 4, 5, 8, 9, 11, 12, 13, 16,
           17, 19, 20, 21, 24, 25, 27, 28, 29, 32,
           33, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537, 2046, 2047, 2048,
           2049, 8191, 8192, 8193, 16383, 16384)
TUNED_D = (13, 27, 1537, 8193)           # mala_tuned / hmc_tuned: one width per family


def family(d):
    return "lpc" if d <= 16 else "lpp" if d <= 32 else "wpc" if d <= 2048 else "bpc"


def expected_step_kernel(d, model, kind, C, uniform_scale):
    """The step kernel instance a run of `kind` on `model` at width d and C chains launches, as
    task.step_kernel reports it."""
    assert model in MODELS and kind in KINDS and 1 <= d <= D_MAX
    b = lambda v: "true" if v else "false"
    nb = -(-d // 4)
    if d <= 32 and kind == "rwm" and C <= LA_MAX_CHAINS:
        if C == 1 and d <= 4:
            return f"lpc_rwm_spec<{d}, {model}, {b(uniform_scale)}>"
        return f"lpc_rwm_la<{nb}, {model}, {b(uniform_scale)}>"
    if d <= 32:
        if d <= 16:
            fam, n, full = "lpc", nb, d % 4 == 0
        else:
            fam, n = "lpp", -(-nb // 2)
            full = d == 8 * n                                  # both lanes hold 4 NBL real coordinates
        head = f"{fam}_{'hmc' if kind == 'hmcda' else kind}<{n}, {b(full and model in FULL_LANE)}, {model}"
        tail = {"rwm": f", {b(uniform_scale)}>", "mala": ">", "hmc": ", false>", "hmcda": ", true>"}[kind]
        return head + tail
    if d <= 2048:
        n = 1
        while 256 * n < d:
            n *= 2
        head = f"wpc_{'hmc' if kind == 'hmcda' else kind}<{n}, {b(d == 256 * n and model in FULL_WAVE)}, {model}"
        return head + {"rwm": ">", "mala": ">", "hmc": ", false>", "hmcda": ", true>"}[kind]
    w = 4 if d <= 8192 else 8
    return f"bpc_{'hmc' if kind == 'hmcda' else kind}<{w}, {model}" + \
        {"rwm": ">", "mala": ">", "hmc": ", false>", "hmcda": ", true>"}[kind]


def edge_positions(d):
    """Coordinates that sit at the corners of the kernel's coordinate -> lane map: 0, d - 1, the first coordinate
    of the last occupied lane slot, and the first coordinate of the last lane (pair kernels), of the last lane of
    the first slot (wave kernels) or of the last wave (block kernels)."""
    nb = -(-d // 4)
    p = {0, d - 1}
    if d <= 16:
        p |= {4 * (nb - 1)}
    elif d <= 32:
        p |= {4 * (-(-nb // 2)), 4 * (nb - 1)}
    elif d <= 2048:
        p |= {252, 256 * ((d - 1) // 256)}
    else:
        w = 4 if d <= 8192 else 8
        p |= {256 * (w - 1), 256 * w * ((d - 1) // (256 * w)), 256 * ((d - 1) // 256)}
    return sorted(q for q in p if 0 <= q < d)


def _u(d):
    """d points of (0.05, 0.95) without an RNG: the central nine tenths of the target's quantile levels.  An init
    spread like a draw from the target keeps the chains near their stationary regime, where step sizes scaled with
    d as below both accept and reject; the tails are left out because a fixed step cannot follow the density's
    local scale next to a support edge (the near-edge coordinates of model() are placed by hand)."""
    return 0.05 + 0.9 * (np.arange(d) + 0.5) / d


def _z(d):
    """the logistic approximation of the standard normal quantile at _u(d)"""
    u = _u(d)
    return np.log(u / (1.0 - u)) / 1.702


def _abs_init(d):                                               # |x| ~ Normal(1, 0.7), signs alternating
    return np.where(np.arange(d) % 2 == 0, 1.0, -1.0) * np.maximum(1.0 + 0.7 * _z(d), 0.05)


def _gamma_init(d, k=2.5, theta=0.7):                           # Wilson-Hilferty
    return k * theta * (1.0 - 1.0 / (9.0 * k) + _z(d) / (3.0 * np.sqrt(k))) ** 3


def _weibull_init(d, k=1.5, lam=2.0):                           # the exact quantile
    return lam * (-np.log1p(-_u(d))) ** (1.0 / k)


# flavour: model name, target, the closed-form init, the target's per-coordinate spread (sets the RWM scale), the
# density's narrowest local scale over the init (sets the MALA / HMC step sizes: next to a support edge the
# curvature (p - 1) / v^2 is what bounds a stable step), the support's edges (None: the whole line)
Flavour = namedtuple("Flavour", "model target init spread gspread lo hi")
FLAVOURS = {
    "iso": Flavour("IsoDot", lambda: mc.IsoNormalDot(), lambda d: np.sqrt(0.5) * _z(d), 0.7, 0.7, None, None),
    "normal": Flavour("NormalDSL", lambda: mc.NormalDSL(0.3, 1.7), lambda d: 0.3 + 1.7 * _z(d), 1.7, 1.7, None, None),
    "abs": Flavour("AbsNormalDSL", lambda: mc.AbsNormalDSL(1.0, 0.7), _abs_init, 0.7, 0.7, None, None),
    "gamma": Flavour("DistDSL", lambda: mc.DistDSL("Gamma", 2.5, 0.7), _gamma_init, 1.1, 0.4, 0.0, None),
    "weibull": Flavour("DistDSL", lambda: mc.DistDSL("Weibull", 1.5, 2.0), _weibull_init, 1.2, 0.4, 0.0, None),
    "beta": Flavour("DistDSL", lambda: mc.DistDSL("Beta", 2.0, 3.0), lambda d: 0.4 + 0.2 * _z(d), 0.2, 0.08, 0.0, 1.0),
}
DIST_FLAVOURS = ("gamma", "weibull", "beta")

Case = namedtuple("Case", "flavour d sampler uniform")


def case_id(c):
    return f"{c.flavour}-d{c.d}-{c.sampler}" + ("-us" if c.uniform and c.d > 1 and c.sampler == "rwm" else "")


def kind_of(sampler):
    return sampler.split("_")[0]


def nchains(c):
    """lpc / lpp: two blocks of the pair and gradient kernels and a tail wave (300); wpc: a tail block of 3 waves
    (67; 11 at the widest); bpc: one block a chain."""
    if family(c.d) == "bpc":
        return 5 if c.sampler in KINDS[:3] else 9               # adapting samplers keep two steps there (runner)
    return 300 if c.d <= 32 else 67 if c.d <= 1024 else 11


# step sizes: RWM scale a / sqrt(d), MALA drift a d^(-1/3), HMC epsilon a d^(-1/4), each times the target's spread
# (its square for the drift, which is a variance)
A_RWM, A_MALA = 1.0, 1.0
A_HMC = {"iso": 0.9, "normal": 0.9}                        # every other flavour: 0.7
HMC_LEAPS = 3
HMCDA_MAX_LEAPS = 6


def jump(c):
    """The proposal's per-coordinate standard deviation (RWM: scale; MALA: sqrt(drift); HMC: epsilon)"""
    f, d, k = FLAVOURS[c.flavour], c.d, kind_of(c.sampler)
    if k == "rwm":
        return A_RWM * f.spread / np.sqrt(d)
    if k == "mala":
        return np.sqrt(A_MALA) * f.gspread * d ** (-1.0 / 6.0)
    return A_HMC.get(c.flavour, 0.7) * f.gspread * d ** -0.25


def sampler(c, store_leaps=False):
    s = jump(c)
    if c.sampler == "rwm":
        return mc.RWM(s)
    if c.sampler == "mala":
        return mc.MALA(s * s)
    if c.sampler == "mala_tuned":
        return mc.MALA(3.0 * s * s, mc.EmpMCTuner(0.6, adaptStep=2))
    if c.sampler == "hmc":
        return mc.HMC(HMC_LEAPS, s, storeLeaps=store_leaps)
    if c.sampler == "hmc_tuned":
        return mc.HMC(HMC_LEAPS, 2.0 * s, mc.EmpMCTuner(0.7, adaptStep=2, maxStep=5), storeLeaps=store_leaps)
    # HMCDA adapts its own epsilon from 1 over the runner's burnin; len sets the trajectory's length.  The block
    # widths' 6 steps leave 3 adapting ones: a sharper shrinkage takes epsilon down to the width's size in those
    return mc.HMCDA(len=HMC_LEAPS * s, max_leaps=HMCDA_MAX_LEAPS, storeLeaps=store_leaps,
                    shrinkage=0.03 if family(c.d) == "bpc" else 0.05)


def runner(c):
    """steps <= 24 below the block-per-chain widths, 6 there.  HMCDA starts every chain at epsilon = 1 and adapts
    while i < burnin: it gets the longer burnin its width allows."""
    da = c.sampler == "hmcda"
    if c.d <= 256:
        return mc.SerialMC(steps=24, burnin=12 if da else 6, thinning=3)
    if c.d <= 2048:
        return mc.SerialMC(steps=24, burnin=14, thinning=2) if da else mc.SerialMC(steps=12, burnin=4, thinning=2)
    return mc.SerialMC(steps=6, burnin=4 if (da or "tuned" in c.sampler) else 1, thinning=1)


EDGE = 1.2     # the near-edge coordinates start this many proposal standard deviations inside the support


def scale_of(c):
    d = c.d
    return 1.0 if c.uniform else np.linspace(0.8, 1.2, d)


def is_uniform(c):
    return bool(c.uniform or c.d == 1)


def model(c):
    """The case's model; DistDSL flavours start a handful of coordinates (edge_positions) close to the support's
    edge -- Beta alternately at its lower and its upper one -- so that some proposals leave the support."""
    f, d = FLAVOURS[c.flavour], c.d
    init = np.array(f.init(d), dtype=np.float64)
    if f.lo is not None:
        off = EDGE * jump(c)
        for n, p in enumerate(edge_positions(d)):
            init[p] = f.hi - off if (f.hi is not None and n % 2 == 1) else f.lo + off
    return mc.MCMCLikelihoodModel(f.target(), init, scale=scale_of(c), gradient=True)


def seed(c):
    return 9000 + 7 * c.d + len(c.flavour) + 13 * KINDS.index(kind_of(c.sampler))


def expected_name(c):
    return expected_step_kernel(c.d, FLAVOURS[c.flavour].model, kind_of(c.sampler), nchains(c), is_uniform(c))


def _cases():
    out = []
    for fl in FLAVOURS:
        non_uniform = fl == "iso"                               # IsoDot with a scale vector, the DSL models' default 1
        for d in D_SWEEP:
            for s in KINDS:
                out.append(Case(fl, d, s, not non_uniform))
                if s == "rwm" and 1 < d <= 32:                  # the lane / pair RWM kernels' other scale instance
                    out.append(Case(fl, d, s, non_uniform))
        for d in TUNED_D:
            out += [Case(fl, d, s, not non_uniform) for s in ("mala_tuned", "hmc_tuned")]
    return out


CASES = _cases()


def all_instances():
    """Every step-kernel name the dispatch can produce for the four models x four sampler kinds at more than
    LA_MAX_CHAINS chains, over d = 1 .. 16384 and both scale kinds (d = 1 has one scale: always uniform)."""
    names = set()
    for d in range(1, D_MAX + 1):
        for m in MODELS:
            for k in KINDS:
                for us in ((True,) if d == 1 else (True, False)):
                    names.add(expected_step_kernel(d, m, k, LA_MAX_CHAINS + 1, us))
    return names


# ------------------------------------------------------------------ device evaluation batches
EVAL_POSITIONS = (0, 3, 4, 255, 256, 4 * 63)


def eval_positions(d):
    return sorted({p for p in EVAL_POSITIONS + (d - 4, d - 1) if 0 <= p < d})


def _in_support(fl, d, n):
    """n in-support columns without an RNG: a Weyl sequence mapped into the flavour's bulk"""
    u = np.modf((np.arange(1, d * n + 1, dtype=np.float64) * 0.6180339887498949).reshape(d, n))[0]
    f = FLAVOURS[fl]
    if f.lo is None:
        return (u - 0.5) * 6.0 * f.spread
    if f.hi is None:
        return 0.1 + 3.9 * u
    return 0.05 + 0.9 * u


SMALLEST_SUBNORMAL = 5e-324


def eval_batch_columns(fl, d):
    """(x [d, n], labels, out-of-support column indices).  Columns: 4 in-support points; DistDSL flavours: one per
    eval position with that coordinate out of the support; then one per (special value, position in {0, d - 1})."""
    f = FLAVOURS[fl]
    base = _in_support(fl, d, 4)
    cols, labels, oos = [base[:, k] for k in range(4)], ["in"] * 4, []
    if f.lo is not None:
        for n, p in enumerate(eval_positions(d)):
            x = base[:, n % 4].copy()
            x[p] = f.hi + 0.25 if (f.hi is not None and n % 2 == 1) else f.lo - 0.25
            oos.append(len(cols))
            cols.append(x)
            labels.append(f"oos@{p}")
    special = [-0.0, np.inf, -np.inf, np.nan, SMALLEST_SUBNORMAL]
    if f.lo is not None:
        special = [f.lo] + ([f.hi] if f.hi is not None else []) + special
    for v in special:
        for p in sorted({0, d - 1}):
            x = base[:, 1].copy()
            x[p] = v
            cols.append(x)
            labels.append(f"{v!r}@{p}")
    return np.ascontiguousarray(np.stack(cols, axis=1)), labels, oos
