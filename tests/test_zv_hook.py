"""The ZV estimators' Julia side and documents, as text (no Julia here): the hook's linearZv / quadraticZv methods for
GPU chains call mcmc_stats_zv with the header's argument list, the plain binding has it too, and the header and the
documents state what is built."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "Int32, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}"


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def _flat(s):
    return re.sub(r"\s+", " ", s)


def test_header_declares_zv():
    h = _read("include", "mcmc_hip.h")
    assert "enum { MCMC_ZV_LINEAR = 1, MCMC_ZV_QUADRATIC = 2 };" in h and "#define MCMC_ABI_VERSION 1" in h
    decl = _flat(h[h.index("int mcmc_stats_zv("):])
    assert decl.startswith("int mcmc_stats_zv(mcmc_ctx* ctx, int32_t order, const double* samples, const double* grads, "
                           "int64_t nkept, int64_t d, int64_t nchains, int32_t on_device, double* zv, double* coef, "
                           "int32_t* info);")
    assert h.index("int mcmc_stats_ess(") < h.index("int mcmc_stats_zv(") < h.index("int mcmc_debug_detmath(")


def test_hook_calls_the_library_for_gpu_chains():
    jl = _read("mcmc.jl_amd", "julia", "mcmc_jl_hook.jl")
    flat = _flat(jl)
    assert "ccall((:mcmc_stats_zv, hiplib), Cint, (Ptr{Void}, " + ARGS + ")" in flat
    assert "linearZv(cs::Array{MCMCChain}) = hip_zv_chains(cs, :linear)" in jl
    assert "quadraticZv(cs::Array{MCMCChain}) = hip_zv_chains(cs, :quadratic)" in jl
    body = jl[jl.index("function hip_zv_chains"):jl.index("linearZv(cs::Array{MCMCChain}) =")]
    assert "isa(c.task.model, MCMCHipModel)" in body and "hip_zv(x, g; order=order" in body
    assert "quadraticZv(c) : linearZv(c)" in body                    # other chains: the reference's own methods
    assert "const HIP_ZV_ORDERS = {:linear => 1, :quadratic => 2}" in jl
    assert "hip_zv" in jl[jl.index("export "):].splitlines()[0]
    # the layouts: samples (C, d, nkept) in, coefficients (C, d, k) out
    assert "Array(Float64, C, d, nk), Array(Float64, C, d, k), Array(Int32, C)" in jl


def test_plain_binding_has_zv():
    jl = _flat(_read("mcmc.jl_amd", "julia", "MCMCHip.jl"))
    assert "ccall((:mcmc_stats_zv, lib), Cint, (Ptr{Cvoid}, " + ARGS + ")" in jl
    assert "function stats_zv(ctx, smp::Array{Float64,3}, grd::Array{Float64,3}; order = 1)" in jl


def test_documents_state_what_is_built():
    readme, integ, design = _read("README.md"), _read("INTEGRATION.md"), _read("DESIGN.md")
    assert "linear_zv" in readme and "zv_device" in readme and "d ≤ 8" in readme
    assert "mcmc_stats_zv" in integ and "linearZv" in integ
    assert "zv.jl" in design[design.index("## 0. Scope"):design.index("## 1. The path")]
    sec = design[design.index("### 5.5"):design.index("### 5.6")]
    for needle in ("k_zv", "Cholesky", "v_mfma_f64_16x16x4_f64", "LDS", "HBM"):
        assert needle in sec, needle
    assert "ZV" in design[design.index("## 4. Summation orders"):design.index("## 5. Kernels")]
    assert os.path.exists(os.path.join(ROOT, "scripts", "zv_probe.py"))
