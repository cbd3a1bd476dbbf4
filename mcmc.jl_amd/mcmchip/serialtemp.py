"""SerialTempMC serial-tempering runner (src/runners/SerialTempMC.jl): many walkers a batch on the GPU.

A walker moves over the tasks' targets: every swapPeriod-th step it resets another task to its position, steps it
once, and switches to it with probability exp(logtarget - logtarget2 + logW[at2] - logW[at]); on other steps it
steps its own task.  Here `nwalkers` independent walkers run at once: walker c is chain c of every target's chain
batch, the sampler steps are the same HIP kernels as SerialMC's, and the pick, take, swap and store run on the device
(kernels/stemp.hip) with no host round trip inside the loop.
"""
from __future__ import annotations

import ctypes as ct
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .api import MCMCChain, MCMCTask, _unpack_bits
from .seqmc import target_seed

__all__ = ["SerialTempMC", "run_serialtempmc", "resume_serialtempmc"]


class _StempCfg(ct.Structure):
    _fields_ = [("steps", ct.c_int64), ("burnin", ct.c_int64), ("swap_period", ct.c_int64)]


class SerialTempMC:
    """SerialTempMC(steps, burnin, swapPeriod) runner (SerialTempMC.jl:16-29)."""

    def __init__(self, steps: int = 1, burnin: int = 0, swapPeriod: int = 5):
        if not burnin >= 0:
            raise AssertionError(f"Burnin rounds ({burnin}) should be >= 0")
        if not steps > burnin:
            raise AssertionError(f"Steps ({steps}) should be > to burnin ({burnin})")
        self.steps, self.burnin, self.swapPeriod = int(steps), int(burnin), int(swapPeriod)

    def cfg(self) -> _StempCfg:
        c = _StempCfg()
        c.steps, c.burnin, c.swap_period = self.steps, self.burnin, self.swapPeriod
        return c


def run_serialtempmc(tasks: Sequence[MCMCTask], nwalkers: Optional[int] = None, logW=None, seed: int = 1,
                     device: int = 0) -> MCMCChain:
    """run(tasks) for SerialTempMC tasks (SerialTempMC.jl:31-85); the runner of the last task sets steps, burnin and
    swapPeriod.  One MCMCChain over the walkers: samples[c] is walker c's [steps - burnin x d] matrix,
    diagnostics["mod"][c] the index into `tasks` of the task it was on at each stored step (the reference's commented
    res.misc[:mod], zero-based here) and diagnostics["swap"][c] whether that step accepted a swap.  logW: the tasks'
    log-weights (default zeros, SerialTempMC.jl:49).  nwalkers defaults to the reference's one.  The chain's task is
    the list of chain batches the walkers ran on; run_serialtempmc(chain.task) continues their step counters."""
    tasks = [t.task if isinstance(t, MCMCChain) else t for t in tasks]
    if not tasks:
        raise ValueError("no tasks")
    d = tasks[-1].model.size
    if not all(t.model.size == d for t in tasks):
        raise AssertionError("Models do not have the same parameter vector size")           # SerialTempMC.jl:39
    runner = tasks[-1].runner
    K = len(tasks)
    w = None if logW is None else np.ascontiguousarray(logW, dtype=np.float64)
    if w is not None and w.shape != (K,):
        raise ValueError(f"logW must have one entry per task ({K})")
    if all(t._h is not None for t in tasks):        # the batches of an earlier run (chain.task): continue them
        if nwalkers is not None and any(t.nchains != int(nwalkers) for t in tasks):
            raise ValueError("started tasks keep their walkers; build new tasks to change nwalkers")
        return _run_on(tasks, runner, w, seed)
    C = 1 if nwalkers is None else int(nwalkers)
    batches = [MCMCTask(t.model, t.sampler, runner, nchains=C, seed=target_seed(seed, k), device=device)
               for k, t in enumerate(tasks)]
    return _run_on(batches, runner, w, seed)


def _run_on(batches, runner, w, seed) -> MCMCChain:
    K, C, d = len(batches), batches[0].nchains, batches[0].model.size
    handles = (ct.c_void_p * K)(*[b.handle() for b in batches])
    nstore = runner.steps - runner.burnin
    samples = np.empty((nstore, d, C))
    mod = np.empty((nstore, C), dtype=np.int32)
    bits = np.zeros((nstore, (C + 63) // 64), dtype=np.uint64)
    final_at = np.empty(C, dtype=np.int32)
    rt = ct.c_double(0.0)
    cfg = runner.cfg()
    _lib.check(_lib.load().mcmc_run_serialtempmc(handles, K, C, ct.byref(cfg), None if w is None else w.ctypes.data,
                                                 ct.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), 0, samples.ctypes.data,
                                                 mod.ctypes.data, bits.ctypes.data, final_at.ctypes.data,
                                                 ct.byref(rt)))
    diags = {"mod": np.ascontiguousarray(mod.T), "swap": _unpack_bits(bits, C), "final_mod": final_at,
             "step": np.arange(runner.burnin + 1, runner.steps + 1)}
    return MCMCChain(range(runner.burnin + 1, runner.steps + 1), samples, None, diags, batches, rt.value)


def resume_serialtempmc(tasks: Sequence[MCMCTask], steps: int = 100, **kw) -> MCMCChain:
    """resume_serialtempmc (SerialTempMC.jl:88-91): the same models and samplers under a new
    SerialTempMC(steps=steps, swapPeriod=...) -- new tasks from model.init, as the reference builds them."""
    tasks = [t.task if isinstance(t, MCMCChain) else t for t in tasks]
    kw.setdefault("nwalkers", tasks[-1].nchains)
    new = [MCMCTask(t.model, t.sampler, SerialTempMC(steps=steps, swapPeriod=t.runner.swapPeriod)) for t in tasks]
    return run_serialtempmc(new, **kw)
