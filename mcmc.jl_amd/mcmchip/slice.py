"""slice_sample (src/samplers/slice_sample.jl:43-112): Neal's univariate-at-a-time slice sampler with stepping out and
shrinkage, for many independent chains of one catalogue model on the GPU (kernels/slice_impl.hpp).

It is a function on a model's log-density, not a sampler: there is no task and no runner.  It asks only for widths,
which there is "little harm in making very large".
"""
from __future__ import annotations

import ctypes as ct
from typing import Optional

import numpy as np

from . import _lib
from .api import MCMCChain, MCMCLikelihoodModel, _draw_chains

__all__ = ["slice_sample", "slice_plan", "slice_last_kernel", "SliceChain"]


class SliceChain(MCMCChain):
    """The MCMCChain of slice_sample.  A scalar `initial` on a d = 1 model with one chain gives `.samples` the
    reference's univariate shape [niter] (slice_sample.jl:109-112); every other call the usual [nchains, niter, d]."""

    univariate = False

    @property
    def samples(self):
        s = np.transpose(self._samples, (2, 0, 1))
        return s.reshape(-1) if self.univariate else s


def _cfg(niter, burnin, iter_begin, step_out, max_evals) -> _lib.SliceCfg:
    c = _lib.SliceCfg()
    c.niter, c.burnin, c.iter_begin = int(niter), int(burnin), int(iter_begin)
    c.step_out, c.max_evals = int(bool(step_out)), int(max_evals)
    return c


def slice_plan(model: MCMCLikelihoodModel, nchains: int = 1):
    """(kernel instance name, threads per block, grid) of slice_sample(model, nchains=nchains); needs no GPU."""
    buf = ct.create_string_buffer(128)
    th, grid = ct.c_int32(0), ct.c_int64(0)
    _lib.check(_lib.load().mcmc_slice_plan(model._desc().kind, model.size, int(nchains), buf, 128, ct.byref(th),
                                           ct.byref(grid)))
    return buf.value.decode(), th.value, grid.value


def slice_last_kernel() -> str:
    """The kernel instance this thread's last slice_sample launched."""
    buf = ct.create_string_buffer(128)
    _lib.check(_lib.load().mcmc_slice_last_kernel(buf, 128))
    return buf.value.decode()


def slice_sample(model: MCMCLikelihoodModel, niter: int, initial=None, widths=None, step_out: bool = True,
                 burnin: int = 0, nchains: int = 1, seed: Optional[int] = None, chain_offset: int = 0,
                 iter_begin: int = 0, max_evals: int = 0, device: int = 0, on_device: bool = False) -> SliceChain:
    """slice_sample(logdist, initial, niter; widths, step_out, burnin) for `nchains` independent chains of `model`.

    initial: None (model.init), a d-vector (every chain starts there), [d, nchains] per-chain starts, or a scalar on a
    d = 1 model.  widths: a d-vector (default ones).  seed None: the chains are drawn from the global stream (srand),
    and chain_offset is not read.  iter_begin: the iterations these chains have run before -- a run of a + b iterations
    is bitwise a run of a, then one of b with iter_begin = a and initial = the first run's final_x.  max_evals: the
    evaluations one coordinate update may spend (0: 4096); a chain that exhausts it stops, diagnostics["info"][c] is the
    iteration, its later rows are NaN.  on_device: samples, final_x, final_lp and info come back as torch tensors on
    the GPU (stats.ess_device / stats.describe_device read the samples in place).

    Returns an MCMCChain: range burnin+1 : burnin+niter, samples [niter][d][nchains], no gradients,
    diagnostics {"info": int32 [nchains], "evals": every log-density evaluation of the run}."""
    lib = _lib.load()
    d, C = model.size, int(nchains)
    cfg = _cfg(niter, burnin, iter_begin, step_out, max_evals)
    _lib.check(lib.mcmc_slice_validate(ct.byref(cfg)))
    univariate = initial is not None and np.ndim(initial) == 0 and d == 1 and C == 1
    init = None
    if initial is not None:
        init = np.asarray(initial.cpu() if hasattr(initial, "cpu") else initial, dtype=np.float64)
        if init.ndim == 0:
            if d != 1:
                raise ValueError(f"a scalar initial needs a d = 1 model (d = {d})")
            init = init.reshape(1)
        if init.shape == (d,):
            init = np.repeat(init[:, None], C, axis=1)
        if init.shape != (d, C):
            raise ValueError(f"initial must be a {d}-vector or [{d}, {C}], got shape {init.shape}")
        init = np.ascontiguousarray(init)
    w = None
    if widths is not None:
        w = np.ascontiguousarray(np.asarray(widths, dtype=np.float64).reshape(-1))
        if w.shape != (d,):
            raise AssertionError(f"widths must have length {d}")                     # slice_sample.jl:49
    if seed is None:
        seed, chain_offset = _draw_chains(C)
    mh = model._handle(device)
    ev, rt, kms = ct.c_int64(0), ct.c_double(0.0), ct.c_double(0.0)
    dinit = None
    if on_device:
        import torch
        dev = torch.device("cuda", device)
        samples = torch.empty((int(niter), d, C), dtype=torch.float64, device=dev)
        fx = torch.empty((d, C), dtype=torch.float64, device=dev)
        flp = torch.empty(C, dtype=torch.float64, device=dev)
        info = torch.empty(C, dtype=torch.int32, device=dev)
        dinit = None if init is None else torch.from_numpy(init).to(dev)
        torch.cuda.synchronize(dev)
        ptr = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
        pinit = None if dinit is None else ptr(dinit)
    else:
        samples, fx, flp = np.empty((int(niter), d, C)), np.empty((d, C)), np.empty(C)
        info = np.empty(C, dtype=np.int32)
        ptr = lambda a: ct.c_void_p(a.ctypes.data)  # noqa: E731
        pinit = None if init is None else ptr(init)
    _lib.check(lib.mcmc_run_slice(mh, ct.byref(cfg), C, int(chain_offset), ct.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                  pinit, None if w is None else ct.c_void_p(w.ctypes.data), int(bool(on_device)),
                                  ptr(samples), ptr(fx), ptr(flp), ptr(info), ct.byref(ev), ct.byref(rt),
                                  ct.byref(kms)))
    diags = {"info": info, "evals": ev.value}
    ch = SliceChain(range(int(burnin) + 1, int(burnin) + int(niter) + 1), samples, None, diags, None, rt.value,
                    kms.value, fx, flp)
    ch.univariate = univariate
    ch.model = model
    return ch
