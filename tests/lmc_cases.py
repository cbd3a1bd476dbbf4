"""Shared ERMLMC / RMLMC cases (test_lmc_cpu.py): the literal tensor C and vxC of the reference from slabs of dG, and a
literal numpy transcription of both samplers (ERMLMC.jl:84-179, RMLMC.jl:89-179) driven by the build's draws."""
import numpy as np

import manifold_ref as lr
import pmala_cases as pc

sr = lr          # the tensor is the same checker's


def literal_C(dG):
    """0.5 (permutedims(dG, [3 2 1]) + permutedims(dG, [1 3 2]) - dG) (ERMLMC.jl:80), dG [d, d, d] with slab r at
    dG[:, :, r]"""
    return 0.5 * (np.transpose(dG, (2, 1, 0)) + np.transpose(dG, (0, 2, 1)) - dG)


def literal_vxC(v, C):
    """vxC[k, :] = v' C[:, :, k] (ERMLMC.jl:116-118)"""
    d = len(v)
    vxC = np.zeros((d, d))
    for k in range(d):
        vxC[k, :] = v @ C[:, :, k]
    return vxC


def _logdet(A):
    sign, ld = np.linalg.slogdet(A)
    assert sign > 0, "logdet of a matrix with a negative determinant"
    return ld


def literal(m, sp, C, steps, seed, burnin):
    """ERMLMC.jl:84-179 or RMLMC.jl:89-179 transcribed with numpy (slabs of dG, np.linalg.inv / cholesky / solve /
    slogdet, libm / scipy), driven by the build's draws; also the smallest margin |ratio - log u| (|ratio| where no
    uniform is drawn) of the accept tests"""
    d = m.size
    tn = sp.tuner
    semi = type(sp).__name__ == "RMLMC"

    def evalalldt(x):
        lp, g, _ = sr.evalallt(m, x.reshape(d, 1))
        return lp[0], g[:, 0], pc.closed_G(m, x), pc.closed_dG(m, x)

    def geometry(G, dG, grad):
        invG = np.linalg.inv(G)
        cholG = np.linalg.cholesky(G).T
        traceInvGxdG = np.array([np.trace(invG @ dG[:, :, i]) for i in range(d)])
        dphi = -grad + 0.5 * traceInvGxdG
        return invG, cholG, dphi, literal_C(dG)
    samples, grads, accs = np.empty((steps, d, C)), np.empty((steps, d, C)), np.zeros((steps, C), dtype=bool)
    margin = np.inf
    sgn = 1.0 if semi else -1.0                                           # RMLMC.jl:110 against ERMLMC.jl:105
    for c in range(C):
        pars = m.init.copy()
        logTarget, grad, G, dG = evalalldt(pars)
        t_nLeaps, t_leapStep, accepted, proposed = sp.nLeaps, sp.leapStep, 0, 0
        for i in range(1, steps + 1):
            if tn is not None:
                proposed += 1
                nLeaps, leapStep = t_nLeaps, t_leapStep
            else:
                nLeaps, leapStep = sp.nLeaps, sp.leapStep
            z, u_acc, u_leaps = lr.draws(seed, c, i, d, "lmc")
            # all geometry from the state's position (the build's set_state departure does not show here: the
            # transcription never resets)
            _, _, G, dG = evalalldt(pars)
            invG, cholG, dphi, Ct = geometry(G, dG, grad)
            proposedPars, proposedG, proposedInvG, proposedCholG = pars.copy(), G, invG, cholG
            proposeddphi, proposedC = dphi, Ct
            velocity = np.linalg.cholesky(proposedInvG) @ z                # (chol(proposedInvG))' * randn
            proposedVelocity = velocity.copy()
            E = -logTarget + sgn * np.sum(np.log(np.diag(cholG))) + 0.5 * velocity @ G @ velocity
            deltaLogDet = 0.0
            nRandomLeaps = int(np.ceil(u_leaps * nLeaps))
            assert nRandomLeaps > 0
            h = leapStep
            for j in range(nRandomLeaps):
                if not semi:
                    vxC = literal_vxC(proposedVelocity, proposedC)
                    deltaLogDet = deltaLogDet - _logdet(proposedG + (0.5 * h) * vxC)
                    proposedVelocity = np.linalg.solve(proposedG + (0.5 * h) * vxC,
                                                       proposedG @ proposedVelocity - (0.5 * h) * proposeddphi)
                    vxC = literal_vxC(proposedVelocity, proposedC)
                    deltaLogDet = deltaLogDet + _logdet(proposedG - (0.5 * h) * vxC)
                else:
                    leapVelocity = proposedVelocity.copy()
                    for k in range(sp.nNewton):
                        vxC = literal_vxC(leapVelocity, proposedC)
                        leapVelocity = proposedVelocity - (0.5 * h) * proposedInvG @ (vxC @ leapVelocity + proposeddphi)
                    proposedVelocity = leapVelocity.copy()
                    deltaLogDet = deltaLogDet - _logdet(proposedG + h * vxC)
                proposedPars = proposedPars + h * proposedVelocity
                proposedLogTarget, proposedGrad, proposedG, proposeddG = evalalldt(proposedPars)
                proposedInvG, proposedCholG, proposeddphi, proposedC = geometry(proposedG, proposeddG, proposedGrad)
                if not semi:
                    vxC = literal_vxC(proposedVelocity, proposedC)
                    deltaLogDet = deltaLogDet - _logdet(proposedG + (0.5 * h) * vxC)
                    proposedVelocity = np.linalg.solve(proposedG + (0.5 * h) * vxC,
                                                       proposedG @ proposedVelocity - (0.5 * h) * proposeddphi)
                    vxC = literal_vxC(proposedVelocity, proposedC)
                    deltaLogDet = deltaLogDet + _logdet(proposedG - (0.5 * h) * vxC)
                else:
                    vxC = literal_vxC(proposedVelocity, proposedC)
                    deltaLogDet = deltaLogDet + _logdet(proposedG - h * vxC)
                    proposedVelocity = proposedVelocity - (0.5 * h) * proposedInvG @ (vxC @ proposedVelocity + proposeddphi)
            proposedE = -proposedLogTarget + sgn * np.sum(np.log(np.diag(proposedCholG))) \
                + 0.5 * proposedVelocity @ proposedG @ proposedVelocity
            ratio = (E - proposedE) + deltaLogDet
            margin = min(margin, abs(ratio) if ratio > 0 else abs(ratio - np.log(u_acc)))
            if ratio > 0 or ratio > np.log(u_acc):
                pars, logTarget, grad = proposedPars.copy(), proposedLogTarget, proposedGrad.copy()
                accs[i - 1, c] = True
                if tn is not None:
                    accepted += 1
            samples[i - 1, :, c], grads[i - 1, :, c] = pars, grad
            if tn is not None and i <= burnin and i % tn.adaptStep == 0:    # adapt!(tune, tuner), HMC.jl:165-169
                rate = accepted / proposed
                t_leapStep *= 1 / (1 + np.exp(-11 * (rate - tn.targetRate))) + 0.5
                t_nLeaps = min(tn.maxStep, int(np.ceil(tn.targetPath / t_leapStep)))
                accepted, proposed = 0, 0
    return samples, grads, accs, margin
