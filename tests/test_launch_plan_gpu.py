"""Full reported instance names of the kernels no other test pins by name: RAM on both sides of every RAM class edge,
NUTS on both sides of the lane / pair edge, and the joint models.  65 chains (past the look-ahead kernels' 64), two
steps; the name from launch_plan_cases.expected_kernel, the samples bitwise against the oracle (oracle_ref.py: RWM,
HMC, RAM; nuts_ref.py: NUTS)."""
import numpy as np
import pytest

import launch_plan_cases as lp
import mcmchip as mc
import nuts_ref as nr
import oracle_ref as orc

pytestmark = pytest.mark.gpu
C = 65
R2 = mc.SerialMC(steps=2)


def _iso(d):
    return mc.model(mc.IsoNormalDot(), init=np.linspace(-0.5, 0.5, d) if d > 1 else np.ones(1), grad=True)


def _normal(d):
    return mc.model(mc.NormalDSL(1, 2), v=np.ones(d), gradient=True)


def _ou():
    m = mc.model(mc.OrnsteinUhlenbeck(mc.ou_series(50)), tau=0.05, sigma=1.0, mu=1.0, gradient=True)
    m.scale = np.array([1000.0, 1.0, 10.0])                                      # ornstein.jl:29-30
    return m


def _distobs():
    return mc.model(mc.DistObsDSL("Normal", 1, 2, v=np.linspace(-1.0, 3.0, 20)), x=1.0, gradient=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(m, sp, model, kind, d, uniform):
    task = (m * sp * R2).batch(C, seed=5)
    chain = mc.run(task)
    assert task.step_kernel == lp.expected_kernel(model, kind, d, C, uniform)
    if kind == "nuts":
        ref = nr.NutsChains(m, sp, C, seed=5).run(R2)["samples"]
    else:
        ref = orc.OracleChains(m, sp, nchains=C, seed=5).run(R2)[0]
    assert chain._samples.shape == ref.shape
    assert np.array_equal(_bits(chain._samples), _bits(ref)), "samples not bit-identical"


@pytest.mark.parametrize("d", [3, 16, 17, 33, 128, 129, 256, 257, 513])
def test_ram_instance_names(gpu, d):
    """lpc_ram<ceil(d/4)> to d = 32; wpc_ram2<1 | 2> to d = 128 | 256; wpc_ram<2 | 4> to d = 512 | 1024"""
    _check(_iso(d), mc.RAM(0.4 / np.sqrt(d)), "IsoDot", "ram", d, True)     # a scale at which some proposals move


@pytest.mark.parametrize("d", [4, 16, 17, 24, 25, 32])
def test_nuts_instance_names(gpu, d):
    """lpc_nuts<NB> to d = 16, lpp_nuts<ceil(NB/2)> to d = 32"""
    _check(_normal(d), mc.NUTS(), "NormalDSL", "nuts", d, True)


@pytest.mark.parametrize("kind,sp", [("rwm", mc.RWM(0.1)), ("ram", mc.RAM()), ("nuts", mc.NUTS())])
def test_ou_instance_names(gpu, kind, sp):
    _check(_ou(), sp, "OUDSL", kind, 3, False)


@pytest.mark.parametrize("kind,sp", [("rwm", mc.RWM(0.1)), ("hmc", mc.HMC(3, 0.05))])
def test_distobs_instance_names(gpu, kind, sp):
    _check(_distobs(), sp, "DistObsDSL", kind, 1, True)
