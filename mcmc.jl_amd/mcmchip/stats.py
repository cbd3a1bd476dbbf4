"""Output analysis of a batched MCMCChain (src/stats/*.jl), vectorised over chains.

acceptance   summary.jl:6-15      100 * sum(accept[lags]) / length(lags)
mean         mean.jl:6
mcvar_iid    var.jl:7-8           var(x) / n
mcvar_bm     var.jl:20-27         batch means
mcvar_imse   var.jl:45-75         Geyer's initial monotone sequence estimator
mcvar_ipse   var.jl:95-117        Geyer's initial positive sequence estimator
var          var.jl:137-149       dispatch on vtype
ess, actime  ess.jl:6-20          n * var_iid / var_vtype, var_vtype / var_iid
linear_zv    zv.jl:8-28           zero-variance estimator, linear control variates
quadratic_zv zv.jl:33-66          zero-variance estimator, quadratic control variates

Autocovariances follow StatsBase.acf(x, lags, correlation=false): the demeaned
sum sum_{t} z_t z_{t+k} / n.  They are computed by FFT over all chains and
parameters at once (the reference loops per column), so values agree with the
reference's direct sums to rounding, not bitwise ("parity unpinned":
StatsBase is not vendored and has no fixture).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

__all__ = ["acceptance", "mean", "mcvar_iid", "mcvar_bm", "mcvar_imse", "mcvar_ipse", "var", "ess", "actime",
           "autocov", "ess_device", "ess_per_sec", "linear_zv", "quadratic_zv", "zv_device", "describe",
           "describe_device", "Describe"]


def _samples(c) -> np.ndarray:
    """[nchains, nkept, d] from an MCMCChain or an array."""
    s = c.samples if hasattr(c, "samples") else np.asarray(c, dtype=np.float64)
    if s.ndim == 1:
        s = s[None, :, None]
    elif s.ndim == 2:
        s = s[None]
    return s


def acceptance(c, lags=None, reject: bool = False) -> np.ndarray:
    """Per-chain acceptance (or rejection) percentage over kept steps `lags` (1-based range)."""
    acc = np.asarray(c.diagnostics["accept"])          # [nchains, nkept] bool
    nk = acc.shape[1]
    if lags is None:
        lags = range(1, nk + 1)
    if not lags[-1] <= nk:
        raise AssertionError("Range of acceptance rate not within post-burnin range of MCMC chain")
    idx = np.asarray(list(lags)) - 1
    rlen = len(idx)
    s = acc[:, idx].sum(axis=1)
    return ((rlen - s) if reject else s) * 100 / rlen


def mean(c) -> np.ndarray:
    return _samples(c).mean(axis=1)


def autocov(x: np.ndarray, maxlag: int) -> np.ndarray:
    """acf(x, 0:maxlag, correlation=false) along axis 1 of x [C, n, d] -> [C, maxlag+1, d]."""
    n = x.shape[1]
    z = x - x.mean(axis=1, keepdims=True)
    nfft = 1
    while nfft < 2 * n:
        nfft *= 2
    f = np.fft.rfft(z, n=nfft, axis=1)
    acv = np.fft.irfft(f * np.conj(f), n=nfft, axis=1)[:, : maxlag + 1] / n
    return acv


def mcvar_iid(c) -> np.ndarray:
    s = _samples(c)
    return s.var(axis=1, ddof=1) / s.shape[1]


def mcvar_bm(c, batchlen: int = 100) -> np.ndarray:
    s = _samples(c)
    nb = s.shape[1] // batchlen
    if not nb > 1:
        raise AssertionError("Choose batch size such that the number of batches is greather than one")
    bm = s[:, : nb * batchlen].reshape(s.shape[0], nb, batchlen, s.shape[2]).mean(axis=2)
    return batchlen * bm.var(axis=1, ddof=1) / (nb * batchlen)


def _geyer(c, maxlag, monotone: bool) -> np.ndarray:
    s = _samples(c)
    n = s.shape[1]
    if maxlag is None:
        maxlag = n - 1
    k = (maxlag - 1) // 2
    acv = autocov(s, maxlag)                                  # [C, maxlag+1, d]
    if 2 * k + 2 > acv.shape[1]:
        acv = np.concatenate([acv, np.zeros((acv.shape[0], 2 * k + 2 - acv.shape[1], acv.shape[2]))], axis=1)
    g = acv[:, 0 : 2 * k + 2 : 2] + acv[:, 1 : 2 * k + 2 : 2]  # g[j] = acv[2j] + acv[2j+1], j = 0..k
    nonpos = g <= 0
    m = np.where(nonpos.any(axis=1), nonpos.argmax(axis=1), k + 1)   # first j with g[j] <= 0, else k+1
    if monotone:
        g = np.minimum.accumulate(g, axis=1)
    j = np.arange(g.shape[1])[None, :, None]
    gs = np.where(j < m[:, None, :], g, 0.0).sum(axis=1)
    return (-acv[:, 0] + 2 * gs) / n


def mcvar_imse(c, maxlag=None) -> np.ndarray:
    return _geyer(c, maxlag, monotone=True)


def mcvar_ipse(c, maxlag=None) -> np.ndarray:
    return _geyer(c, maxlag, monotone=False)


def var(c, vtype: str = "imse", **kw) -> np.ndarray:
    vt = vtype.lstrip(":")
    if vt not in ("bm", "iid", "imse", "ipse"):
        raise AssertionError(f"Unknown variance type {vtype}")
    return {"bm": mcvar_bm, "iid": mcvar_iid, "imse": mcvar_imse, "ipse": mcvar_ipse}[vt](c, **kw)


def ess(c, vtype: str = "imse", **kw) -> np.ndarray:
    """Effective sample size per chain and parameter (ess.jl:6-10)."""
    vt = vtype.lstrip(":")
    if vt not in ("bm", "imse", "ipse"):
        raise AssertionError(f"Unknown ESS type {vtype}")
    n = _samples(c).shape[1]
    return n * var(c, "iid") / var(c, vt, **kw)


def actime(c, vtype: str = "imse", **kw) -> np.ndarray:
    """Integrated autocorrelation time (ess.jl:13-17)."""
    vt = vtype.lstrip(":")
    if vt not in ("bm", "imse", "ipse"):
        raise AssertionError(f"Unknown integrated autocorrelation time type {vtype}")
    return var(c, vt, **kw) / var(c, "iid")


_VT = {"imse": 1, "ipse": 2, "bm": 3}


def ess_device(c, vtype: str = "imse", maxlag: Optional[int] = None, batchlen: int = 100, device: int = 0,
               return_var: bool = False):
    """ESS of every (chain, parameter) series on the GPU (kernels/stats.hip; ess.jl:6-10).

    `c` is an MCMCChain (host samples; returns numpy [nchains, d] like `ess`) or a device tensor
    [nkept, d, nchains] in the C-ABI layout (returns a device tensor [d, nchains], nothing crosses PCIe)."""
    import ctypes as ct
    from . import _lib
    from .api import _ctx
    vt = vtype.lstrip(":")
    if vt not in _VT:
        raise AssertionError(f"Unknown ESS type {vtype}")
    lib = _lib.load()
    ml = 0 if maxlag is None else int(maxlag)
    if hasattr(c, "data_ptr"):                                   # torch device tensor
        import torch
        if c.dim() != 3 or c.dtype != torch.float64 or not c.is_contiguous():
            raise ValueError("expected a contiguous float64 tensor [nkept, d, nchains]")
        n, d, C = c.shape
        e = torch.empty((d, C), dtype=torch.float64, device=c.device)
        v = torch.empty((d, C), dtype=torch.float64, device=c.device) if return_var else None
        _lib.check(lib.mcmc_stats_ess(_ctx(c.device.index or 0), c.data_ptr(), n, d, C, _VT[vt], ml, batchlen, 1,
                                      e.data_ptr(), v.data_ptr() if v is not None else None))
        return (e, v) if return_var else e
    s = np.ascontiguousarray(c._samples if hasattr(c, "_samples") else c, dtype=np.float64)
    n, d, C = s.shape
    e = np.empty((d, C))
    v = np.empty((d, C)) if return_var else None
    _lib.check(lib.mcmc_stats_ess(_ctx(device), s.ctypes.data, n, d, C, _VT[vt], ml, batchlen, 0, e.ctypes.data,
                                  v.ctypes.data if v is not None else None))
    return (e.T.copy(), v.T.copy()) if return_var else e.T.copy()


class Describe:
    """What describe / describe_device return.

    per_chain   the six columns `columns` = (min, mean, max, mcerror, ess, actime) of every series: numpy
                [nchains, d, 6] from host samples, a device tensor [6, d, nchains] (the C-ABI layout) from a device
                tensor, None when not asked for; column(name) [nchains, d] and table() (numpy [nchains, d, 6]) read
                either the same way
    pooled     {min, mean, max, mcerror, ess, rhat} -> [d]
    quantiles   [nprobs, d], the exact pooled quantiles at `probs`
    nbad        [d]: the chains left out of the pooled mcerror and ess"""
    columns = ("min", "mean", "max", "mcerror", "ess", "actime")
    rows = ("min", "mean", "max", "mcerror", "ess", "rhat")

    def __init__(self, per_chain, pooled, quantiles, probs, nbad):
        self.per_chain, self.pooled, self.quantiles, self.probs, self.nbad = per_chain, pooled, quantiles, probs, nbad

    def column(self, name):
        """one column of the per-chain table as [nchains, d] whichever path produced it: a numpy view, or a view of
        the device tensor (nothing is copied)"""
        i = self.columns.index(name)
        return self.per_chain[i].T if hasattr(self.per_chain, "data_ptr") else self.per_chain[:, :, i]

    def table(self) -> np.ndarray:
        """the per-chain table as numpy [nchains, d, 6] whichever path produced it (a device table is copied to the
        host: 48 bytes a series)"""
        if hasattr(self.per_chain, "data_ptr"):
            return np.ascontiguousarray(self.per_chain.cpu().numpy().transpose(2, 1, 0))
        return self.per_chain

    def write_pooled(self, io, names=None) -> None:
        """the pooled rows and quantiles of every parameter, in the layout of the reference's per-chain table"""
        host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
        rows = {nm: host(v) for nm, v in self.pooled.items()}
        q, nbad = host(self.quantiles), host(self.nbad)
        labels = dict(zip(self.rows, ("Min", "Mean", "Max", "MC Error", "ESS", "Rhat")))
        for j in range(len(nbad)):
            print(f"{names[j] if names else f'x{j + 1}'} (pooled, {int(nbad[j])} chain(s) left out of MC Error and ESS)",
                  file=io)
            for nm in self.rows:
                print(f"{labels[nm]:<10} {float(rows[nm][j])!r}", file=io)
            for p, row in zip(self.probs, q):
                print(f"{'Q ' + repr(p):<10} {float(row[j])!r}", file=io)
            print(file=io)


def _quantile7(v_sorted: np.ndarray, p: float) -> float:
    """Julia's quantile (type 7) on sorted values, plain multiply and add"""
    N = len(v_sorted)
    h = np.float64(N - 1) * np.float64(p)
    lo = int(np.floor(h))
    f = h - np.floor(h)
    vlo = v_sorted[lo]
    return vlo + f * (v_sorted[min(lo + 1, N - 1)] - vlo)


def describe(c, io=None, probs=(0.025, 0.5, 0.975), maxlag=None) -> Describe:
    """describe(c) (summary.jl:24-55) in numpy: per chain and parameter Min, Mean, Max, MC Error, ESS, AC Time exactly as
    the reference forms them from mcvar_imse and var, plus the pooled rows and quantiles describe_device gives.  For
    one chain the reference's table is printed (to `io`, default stdout); for more, only when `io` is given."""
    import sys
    s = _samples(c)                                            # [C, n, d]
    C, n, d = s.shape
    with np.errstate(all="ignore"):
        varimse = mcvar_imse(s, maxlag)                        # summary.jl:38
        variid = s.var(axis=1, ddof=1) / n                     # :39
        mcerror = np.sqrt(varimse)                             # :40
        ss = n * variid / varimse                              # :41
        act = varimse / variid                                 # :42
        mn, mx, mean_ = s.min(axis=1) + 0.0, s.max(axis=1) + 0.0, s.mean(axis=1)
        per_chain = np.stack([mn, mean_, mx, mcerror, ss, act], axis=2)
        good = np.isfinite(varimse) & np.isfinite(ss) & (varimse > 0)
        ngood = good.sum(axis=0)
        W = s.var(axis=1, ddof=1).mean(axis=0)
        Bn = mean_.var(axis=0, ddof=1) if C > 1 else np.full(d, np.nan)
        rhat = np.where((C > 1) & (W != 0), np.sqrt(((n - 1) / n * W + Bn) / np.where(W != 0, W, 1.0)), np.nan)
        pooled = {"min": mn.min(axis=0), "mean": mean_.mean(axis=0), "max": mx.max(axis=0),
                  "mcerror": np.sqrt(np.where(good, varimse, 0.0).sum(axis=0)) / ngood,
                  "ess": np.where(good, ss, 0.0).sum(axis=0), "rhat": rhat}
        flat = np.sort(s.reshape(C * n, d) + 0.0, axis=0)
        q = np.array([[_quantile7(flat[:, j], p) for j in range(d)] for p in probs]).reshape(len(probs), d)
    if io is None and C == 1:
        io = sys.stdout
    if io is not None:
        names = getattr(c, "names", None) or [f"x{j + 1}" for j in range(d)]
        for ch in range(C):
            for j in range(d):
                print(names[j] if C == 1 else f"{names[j]} (chain {ch + 1})", file=io)
                for nm, v in zip(("Min", "Mean", "Max", "MC Error", "ESS", "AC Time"), per_chain[ch, j]):
                    print(f"{nm:<10} {v!r}" if not isinstance(v, np.floating) else f"{nm:<10} {float(v)!r}", file=io)
                print("NAs        0", file=io)
                print("NA%        0.0%", file=io)
                print(file=io)
    return Describe(per_chain, pooled, q, tuple(probs), (C - ngood).astype(np.int64))


def describe_device(c, probs=(0.025, 0.5, 0.975), maxlag: Optional[int] = None, device: int = 0,
                    per_chain: bool = True, pooled: bool = True) -> Describe:
    """describe on the GPU (kernels/describe.hip; mcmc_stats_describe): the per-chain table in one read of the samples,
    the pooled rows from the per-chain values, exact pooled quantiles by radix select.

    `c` is an MCMCChain (host samples: numpy results, the per-chain table [nchains, d, 6]) or a device tensor
    [nkept, d, nchains] in the C-ABI layout (device tensors: the table [6, d, nchains], the pooled rows [d], the
    quantiles [nprobs, d], nbad [d]; nothing but the few probabilities crosses PCIe)."""
    from . import _lib
    from .api import _ctx
    lib = _lib.load()
    ml = 0 if maxlag is None else int(maxlag)
    probs = tuple(float(p) for p in probs)
    npr, NP = len(probs), len(Describe.rows)
    if hasattr(c, "data_ptr"):
        import torch
        if c.dim() != 3 or c.dtype != torch.float64 or not c.is_contiguous():
            raise ValueError("expected a contiguous float64 tensor [nkept, d, nchains]")
        n, d, C = c.shape
        kw = dict(dtype=torch.float64, device=c.device)
        pc = torch.empty((6, d, C), **kw) if per_chain else None
        po = torch.empty((NP + npr, d), **kw) if pooled else None
        nb = torch.empty((d,), dtype=torch.int64, device=c.device) if pooled else None
        pr = torch.tensor(probs, **kw) if pooled and npr else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.check(lib.mcmc_stats_describe(_ctx(c.device.index or 0), c.data_ptr(), n, d, C, ml, 1, ptr(pc), ptr(pr),
                                           npr, ptr(po), ptr(nb)))
    else:
        s = np.ascontiguousarray(c._samples if hasattr(c, "_samples") else c, dtype=np.float64)
        if s.ndim != 3:
            raise ValueError("expected samples [nkept, d, nchains]")
        n, d, C = s.shape
        pc = np.empty((6, d, C)) if per_chain else None
        po = np.empty((NP + npr, d)) if pooled else None
        nb = np.empty(d, dtype=np.int64) if pooled else None
        pr = np.array(probs, dtype=np.float64)
        ptr = lambda a: a.ctypes.data if a is not None else None
        _lib.check(lib.mcmc_stats_describe(_ctx(device), s.ctypes.data, n, d, C, ml, 0, ptr(pc), ptr(pr) if npr else None,
                                           npr, ptr(po), ptr(nb)))
        if pc is not None:
            pc = np.ascontiguousarray(pc.transpose(2, 1, 0))   # [nchains, d, 6], as describe's
    rows = {nm: po[i] for i, nm in enumerate(Describe.rows)} if po is not None else None
    return Describe(pc, rows, po[NP:] if po is not None else None, probs, nb)


def ess_per_sec(ess_dc, seconds: float) -> float:
    """sum over chains of min over parameters of ESS, per sampling second."""
    m = ess_dc.min(dim=0).values.sum().item() if hasattr(ess_dc, "min") and hasattr(ess_dc, "dim") \
        else float(np.min(ess_dc, axis=0).sum())
    return m / seconds


def _samples_grads(c, grad=None):
    """([C, nkept, d] samples, gradients) of an MCMCChain, or of two arrays."""
    if grad is None:
        if getattr(c, "_gradients", 0) is None or getattr(c, "gradients", None) is None:
            raise ValueError("ZV estimators need the chain's gradients: run a gradient sampler (MALA, HMC, HMCDA, "
                             "NUTS) with store_gradients on")
        grad = c.gradients
    s, g = _samples(c), _samples(grad)
    if s.shape != g.shape:
        raise ValueError(f"samples {s.shape} and gradients {g.shape} differ in shape")
    return s, g


def _zv(x: np.ndarray, w: np.ndarray):
    """zv.jl:18-25 / :55-63 for one chain: x [n, d], control variates w [n, k] -> (x + w a, a [k, d])."""
    d, k = x.shape[1], w.shape[1]
    a = np.empty((k, d))
    for i in range(d):
        cov_all = np.atleast_2d(np.cov(np.column_stack([w, x[:, i]]), rowvar=False))
        precision = np.linalg.inv(cov_all[:k, :k])
        sigma = cov_all[:k, k]
        a[:, i] = -precision @ sigma
    return x + w @ a, a


def linear_zv(c, grad=None):
    """linearZv (zv.jl:8-30) per chain: (zv_chain [C, nkept, d], a [C, d, d])."""
    s, g = _samples_grads(c, grad)
    out = [_zv(x, -gr / 2) for x, gr in zip(s, g)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def quadratic_zv(c, grad=None):
    """quadraticZv (zv.jl:33-68) per chain: (zv_chain [C, nkept, d], a [C, d(d+3)/2, d])."""
    s, g = _samples_grads(c, grad)
    out = []
    for x, gr in zip(s, g):
        n, d = x.shape
        z = -gr / 2
        zq = np.empty((n, d * (d + 3) // 2))
        zq[:, :d] = z
        zq[:, d:2 * d] = 2 * z * x - 1
        col = 2 * d
        for i in range(d - 1):
            for j in range(i + 1, d):
                zq[:, col] = x[:, i] * z[:, j] + x[:, j] * z[:, i]
                col += 1
        out.append(_zv(x, zq))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def zv_device(c, order: int = 1, device: int = 0, return_coef: bool = False, return_info: bool = False):
    """ZV estimators of every chain on the GPU (kernels/zv.hip; zv.jl:8-68); order 1 linear, 2 quadratic.

    `c` is an MCMCChain (host arrays; returns numpy [nchains, nkept, d] like `samples`, coefficients
    [nchains, k, d], info [nchains]) or a pair (samples, gradients) of contiguous float64 device tensors
    [nkept, d, nchains] in the C-ABI layout (returns device tensors [nkept, d, nchains], [k, d, nchains], [nchains];
    nothing crosses PCIe, and the result can go straight into `ess_device`).  info[c] != 0 marks a chain whose Gram
    matrix is not positive definite; its values are NaN."""
    from . import _lib
    from .api import _ctx
    if order not in (1, 2):
        raise ValueError(f"Unknown ZV order {order}: 1 (linear) or 2 (quadratic)")
    lib = _lib.load()

    def pack(z, a, i):
        out = (z,) + ((a,) if return_coef else ()) + ((i,) if return_info else ())
        return out if len(out) > 1 else z

    if isinstance(c, (tuple, list)) and len(c) == 2 and hasattr(c[0], "data_ptr"):
        import torch
        x, g = c
        for t in (x, g):
            if t.dim() != 3 or t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("expected contiguous float64 device tensors [nkept, d, nchains]")
        if x.shape != g.shape or x.device != g.device:
            raise ValueError("samples and gradients differ in shape or device")
        n, d, C = x.shape
        k = d * (d + 3) // 2 if order == 2 else d
        z = torch.empty_like(x)
        a = torch.empty((k, d, C), dtype=torch.float64, device=x.device) if return_coef else None
        i = torch.empty((C,), dtype=torch.int32, device=x.device) if return_info else None
        _lib.check(lib.mcmc_stats_zv(_ctx(x.device.index or 0), order, x.data_ptr(), g.data_ptr(), n, d, C, 1,
                                     z.data_ptr(), a.data_ptr() if a is not None else None,
                                     i.data_ptr() if i is not None else None))
        return pack(z, a, i)
    if hasattr(c, "_samples"):
        if getattr(c, "_gradients", None) is None:
            raise ValueError("ZV estimators need the chain's gradients: run a gradient sampler (MALA, HMC, HMCDA, "
                             "NUTS) with store_gradients on")
        x, g = c._samples, c._gradients
    else:
        x, g = c
    x = np.ascontiguousarray(x, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    if x.ndim != 3 or x.shape != g.shape:
        raise ValueError("expected samples and gradients [nkept, d, nchains] of one shape")
    n, d, C = x.shape
    k = d * (d + 3) // 2 if order == 2 else d
    z = np.empty((n, d, C))
    a = np.empty((k, d, C)) if return_coef else None
    i = np.empty(C, dtype=np.int32) if return_info else None
    _lib.check(lib.mcmc_stats_zv(_ctx(device), order, x.ctypes.data, g.ctypes.data, n, d, C, 0, z.ctypes.data,
                                 a.ctypes.data if a is not None else None, i.ctypes.data if i is not None else None))
    return pack(np.ascontiguousarray(z.transpose(2, 0, 1)),
                np.ascontiguousarray(a.transpose(2, 0, 1)) if a is not None else None, i)
