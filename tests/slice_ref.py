"""A literal Python transcription of slice_sample (src/samplers/slice_sample.jl:43-103) -- TEST INFRASTRUCTURE ONLY.

Line for line the reference's function for one chain: it keeps the vector copies x_l, x_r and xprime and its three
while loops.  rand() is draw k = 0, 1, 2, ... of the update (iter, dd) from the project's counter-based stream (the
checker's orc_slice_draw), log is the oracle's, and logdist is the oracle's batch eval of the whole vector.  The two
places where the reference would loop without end or assert raise Stop instead (include/mcmc_hip.h, mcmc_run_slice).
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

import oracle_ref as orc
import slice_cases as sc


class Stop(Exception):
    pass


class LogDist:
    """logdist(x): one oracle eval of the d-vector, counted; the budget of one coordinate update"""

    def __init__(self, m, max_evals):
        self.om = orc.OracleModel(m)
        self.order = orc.kernel_order(m)
        self.d = m.size
        self.lp = np.empty(1)
        self.g = np.empty(m.size)
        self.max_evals = max_evals
        self.total = 0
        self.used = 0

    def __call__(self, x, budget=True):
        if budget:
            if self.used >= self.max_evals:
                raise Stop()
            self.used += 1
        self.total += 1
        xs = np.ascontiguousarray(x, dtype=np.float64)
        orc.lib().orc_eval_batch(ct.byref(self.om.s), 1, orc._d(xs), orc._d(self.lp), orc._d(self.g), self.order)
        return float(self.lp[0])


def slice_sample_chain(m, initial, niter, widths, step_out=True, burnin=0, seed=1, chain=0, iter_begin=0,
                       max_evals=sc.DEFAULT_EVALS):
    """(history [niter][d], final state, final log_Px, info, evaluations) of one chain"""
    L = sc.checker()
    logdist = LogDist(m, max_evals)
    D = len(initial)
    assert len(widths) == D                                                     # :49
    state = np.array(initial, dtype=np.float64)                                 # :51
    log_Px = logdist(state, budget=False)                                       # :52
    history = np.zeros((niter, D))                                              # :54
    info = 0
    for it in range(1, niter + burnin + 1):                                     # :56
        itr = iter_begin + it
        if info == 0:
            saved, saved_lp = state.copy(), log_Px
            try:
                for dd in range(D):                                             # :62
                    k = [0]

                    def rand():
                        u = L.orc_slice_draw(ct.c_uint64(seed), chain, itr, dd, k[0])
                        k[0] += 1
                        return u

                    logdist.used = 0
                    log_uprime = L.orc_slice_log(rand()) + log_Px               # :63
                    x_l = state.copy()                                          # :64
                    x_r = state.copy()                                          # :65
                    xprime = state.copy()                                       # :66
                    r = rand()                                                  # :68
                    x_l[dd] = state[dd] - np.float64(r) * widths[dd]            # :69
                    x_r[dd] = state[dd] + (np.float64(1) - np.float64(r)) * widths[dd]   # :70
                    if step_out:                                                # :71
                        while logdist(x_l) > log_uprime:                        # :72
                            x_l[dd] -= widths[dd]                               # :73
                        while logdist(x_r) > log_uprime:                        # :75
                            x_r[dd] += widths[dd]                               # :76
                    while True:                                                 # :81
                        xprime[dd] = np.float64(rand()) * (x_r[dd] - x_l[dd]) + x_l[dd]   # :82
                        log_Px = logdist(xprime)                                # :83
                        if log_Px > log_uprime:                                 # :84
                            break
                        elif xprime[dd] > state[dd]:                            # :87
                            x_r[dd] = xprime[dd]
                        elif xprime[dd] < state[dd]:                            # :89
                            x_l[dd] = xprime[dd]
                        else:
                            raise Stop()                                        # :92
                    state[dd] = xprime[dd]                                      # :96
            except Stop:
                info = it
                state, log_Px = saved, saved_lp
        if it > burnin:                                                         # :98
            history[it - burnin - 1, :] = np.nan if info else state             # :99
    return history, state, log_Px, info, logdist.total
