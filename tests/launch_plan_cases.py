"""The step-kernel instance of every target of the separable and joint family, restated from the model, the sampler,
d and C alone (not read from the library): separable_cases.expected_step_kernel for the four separable models under
RWM / MALA / HMC / HMCDA, and here RAM, NUTS and the two joint models (DistObsDSL, OUDSL: lane and pair kernels only,
no FULL instances).  test_launch_plan_cpu.py compares the library's launch plan with it on the CPU,
test_launch_plan_gpu.py what a run reports.  launch_shape lists, by family, the block sizes the hand-written launch
sites had before the plan replaced them.
"""
import separable_cases as sc

JOINT = ("DistObsDSL", "OUDSL")
MODELS = sc.MODELS + JOINT
SAMPLERS = sc.KINDS + ("ram", "nuts")
LPC_MAX_D, RAM_MAX_D, NUTS_MAX_D = 32, 1024, 32
NUTS_JOINT_MAX_D = 4                                   # the joint models' NUTS is built for one Philox block: d <= 4


def _b(v):
    return "true" if v else "false"


def expected_kernel(model, kind, d, C, uniform_scale):
    """task.step_kernel of a run of `kind` on `model` at width d and C chains; None where the library refuses."""
    assert model in MODELS and kind in SAMPLERS
    nb = -(-d // 4)
    if d < 1 or d > (LPC_MAX_D if model in JOINT else sc.D_MAX):
        return None
    if kind == "ram":
        if model == "DistObsDSL" or d > RAM_MAX_D:
            return None
        if d <= 32:
            return f"lpc_ram<{nb}, {model}>"
        if d <= 256:
            return f"wpc_ram2<{1 if d <= 128 else 2}, {model}>"
        return f"wpc_ram<{2 if d <= 512 else 4}, {model}>"
    if kind == "nuts":
        if d > (NUTS_JOINT_MAX_D if model in JOINT else NUTS_MAX_D):
            return None
        return f"lpc_nuts<{nb}, {model}>" if d <= 16 else f"lpp_nuts<{-(-nb // 2)}, {model}>"
    if model in sc.MODELS:
        return sc.expected_step_kernel(d, model, kind, C, uniform_scale)
    # joint models: expected_step_kernel's lane and pair branches with F = false
    if kind == "rwm" and C <= sc.LA_MAX_CHAINS:
        if C == 1 and d <= 4:
            return f"lpc_rwm_spec<{d}, {model}, {_b(uniform_scale)}>"
        return f"lpc_rwm_la<{nb}, {model}, {_b(uniform_scale)}>"
    fam, n = ("lpc", nb) if d <= 16 else ("lpp", -(-nb // 2))
    tail = {"rwm": f", {_b(uniform_scale)}>", "mala": ">", "hmc": ", false>", "hmcda": ", true>"}[kind]
    return f"{fam}_{'hmc' if kind == 'hmcda' else kind}<{n}, false, {model}" + tail


def expected_aux_kernel(model, op, kind, d):
    """The eval, storeLeaps-record and NUTS-init instances (they report no name; the plan formats one all the same)."""
    nb = -(-d // 4)
    if op == "init":
        name = expected_kernel(model, "nuts", d, 65, True)
        return name and name.replace("_nuts<", "_nuts_init<")
    if d < 1 or d > (LPC_MAX_D if model in JOINT else sc.D_MAX):
        return None
    if d <= 32:
        fam, n = ("lpc", nb) if d <= 16 else ("lpp", -(-nb // 2))
    elif d <= 2048:
        fam, n = "wpc", [k for k in (1, 2, 4, 8) if d <= 256 * k][0]
    else:
        fam, n = "bpc", 4 if d <= 8192 else 8
    return f"{fam}_eval<{n}, {model}>" if op == "eval" else f"{fam}_hmc_rec<{n}, {model}, {_b(kind == 'hmcda')}>"


def launch_shape(name):
    """(threads per block, chains per block) of the launch site of the instance `name`; chains per block
    None: a single block (the look-ahead and speculation kernels)."""
    fam, args = name.split("<")
    args = args.rstrip(">").split(", ")
    n = int(args[0])
    if fam in ("lpc_rwm_la", "lpc_rwm_spec"):
        return 256, None
    if fam == "lpc_rwm":
        return 512, 512
    if fam in ("lpc_mala", "lpc_hmc"):
        t = {1: 512, 2: 768, 3: 256, 4: 256}[n]
        return t, t
    if fam in ("lpp_rwm", "lpp_hmc"):
        return 512, 256
    if fam == "lpp_mala":
        t = 768 if args[1] == "true" else 512
        return t, t // 2
    if fam in ("lpc_ram", "lpc_nuts", "lpc_nuts_init", "lpc_eval", "lpc_hmc_rec"):
        return 256, 256
    if fam in ("lpp_nuts", "lpp_nuts_init", "lpp_eval", "lpp_hmc_rec"):
        return 256, 128
    if fam == "wpc_ram2":
        return 256, 8
    if fam.startswith("wpc_"):
        return 256, 4
    assert fam.startswith("bpc_"), name
    return 64 * n, 1
