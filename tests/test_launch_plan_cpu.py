"""The launch plan of the separable and joint targets (csrc/kernels/launch_plan.hpp) is plain C++: a stand-alone
program walks it under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU, and its lines are compared with the
restatements in separable_cases.py and launch_plan_cases.py."""
import functools
import os
import subprocess
import tempfile

import launch_plan_cases as lp
import separable_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
CS = (1, 2, 64, 65, 127, 128, 129, 1 << 20)
DS = sorted(set(range(1, 41)) | set(sc.D_SWEEP))
N_STEP = len(lp.MODELS) * len(lp.SAMPLERS) * len(DS) * len(CS) * 2
N_AUX = len(lp.MODELS) * len(DS) * len(CS) * 4


@functools.lru_cache(maxsize=None)
def walk():
    """the program's output, computed once and shared: (step lines, further lines), each
    (op, model, sampler, d, C, us, built, grid, threads, chains per block, name)"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "launch_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "launch_plan_check.cpp")], check=True)
        r = subprocess.run([exe] + [str(d) for d in sc.D_SWEEP], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert f"{N_STEP} combinations\n" in r.stdout and f"{N_AUX} further plans\n" in r.stdout
    assert "0 plans built outside the family" in r.stdout
    rows = []
    for ln in r.stdout.splitlines():
        f = ln.split(" ", 10)
        if f[0] in ("step", "eval", "record", "init"):
            rows.append((f[0], f[1], f[2]) + tuple(int(v) for v in f[3:10]) + (f[10],))
    step = tuple(w for w in rows if w[0] == "step")
    return step, tuple(w for w in rows if w[0] != "step")


def test_walk_covers_every_combination():
    step, aux = walk()
    assert N_STEP == 6 * 6 * 59 * 8 * 2 and len(step) == N_STEP and len(aux) == N_AUX
    assert {(w[1], w[2], w[3], w[4], w[5]) for w in step} == \
        {(m, s, d, C, us) for m in lp.MODELS for s in lp.SAMPLERS for d in DS for C in CS for us in (0, 1)}


def test_separable_names_are_the_tables():
    """the four separable models under RWM / MALA / HMC / HMCDA: separable_cases.expected_step_kernel"""
    n = 0
    for _, model, kind, d, C, us, built, _, _, _, name in walk()[0]:
        if model in sc.MODELS and kind in sc.KINDS:
            assert built and name == sc.expected_step_kernel(d, model, kind, C, bool(us)), (model, kind, d, C, us, name)
            n += 1
    assert n == 4 * 4 * len(DS) * len(CS) * 2


def test_ram_nuts_and_joint_names_and_refusals():
    """every combination: built exactly where the restatement has a name, and then that name"""
    refused = 0
    for _, model, kind, d, C, us, built, _, _, _, name in walk()[0]:
        want = lp.expected_kernel(model, kind, d, C, bool(us))
        assert (name if built else None) == want, (model, kind, d, C, us, name, want)
        refused += not built
    assert refused > 0
    for op, model, kind, d, C, _, built, _, _, _, name in walk()[1]:
        assert (name if built else None) == lp.expected_aux_kernel(model, op, kind, d), (op, model, kind, d, name)


def test_grid_covers_the_chains_exactly():
    for w in walk()[0] + walk()[1]:
        C, built, grid, cpb = w[4], w[6], w[7], w[9]
        if built:
            assert grid * cpb >= C > (grid - 1) * cpb, w


def test_block_sizes_are_the_launch_sites():
    for w in walk()[0] + walk()[1]:
        built, grid, threads, cpb, name = w[6], w[7], w[8], w[9], w[10]
        if built:
            t, c = lp.launch_shape(name)
            assert threads == t and (grid == 1 if c is None else cpb == c), w
