// layout_api.hpp -- what the per-model kernel units (lpc_<model>.hip, lpc_ram_*.hip, wpc_<model>.hip, wpc_ram.hip,
// nuts_<model>.hip) export, the unit tables of lpc.hip / wpc.hip / nuts.hip, and the instance dispatcher: every launch
// of the family runs the instance launch_plan.hpp names.
#pragma once
#include <type_traits>

#include "../host/kernels_api.hpp"
#include "launch_plan.hpp"

namespace mcmc {

// One unit's entries; an entry the unit does not build is null.  RAM and NUTS units have the step entry alone (NUTS:
// the plan says whether it is the step loop or the initial epsilon search).
struct KernelUnit {
    hipError_t (*step)(const KernelArgs& a, const LaunchPlan& p, hipStream_t st);
    hipError_t (*eval)(const KernelArgs& a, const LaunchPlan& p, const double* xin, double* lp, double* g, int check,
                       hipStream_t st);
    hipError_t (*record)(const KernelArgs& a, const LaunchPlan& p, const LeapRec& r, hipStream_t st);
};
using UnitFn = KernelUnit();          // a unit's export: its entries
UnitFn lpc_iso, lpc_normal, lpc_absnormal, lpc_dist, lpc_distobs, lpc_ou;
UnitFn lpc_ram_iso, lpc_ram_normal, lpc_ram_absnormal, lpc_ram_dist, lpc_ram_ou;
UnitFn wpc_iso, wpc_normal, wpc_absnormal, wpc_dist;
UnitFn wpc_ram_iso, wpc_ram_normal, wpc_ram_absnormal, wpc_ram_dist;
UnitFn nuts_iso, nuts_normal, nuts_absnormal, nuts_dist, nuts_distobs, nuts_ou;
// the slice units (slice_<model>.hip) export their one launcher; slice.hip's table holds them
using SliceFn = hipError_t(const SliceKernelArgs& a, const LaunchPlan& p, hipStream_t st);
SliceFn slice_iso, slice_normal, slice_absnormal, slice_dist, slice_distobs, slice_ou;

// a mapping's table: one row per model kind; a null unit, like a null entry, is refused with hipErrorInvalidValue
struct UnitRow {
    int32_t kind;
    UnitFn* unit;
    UnitFn* ram;
};
// The launch's plan and the unit that runs it; no entries when the combination is not built, or is not one of this
// table's state layout (wave: [C][ld], d > kPairMaxD).
template <size_t N>
static KernelUnit unit_for(const UnitRow (&rows)[N], const KernelArgs& a, PlanOp op, bool wave, LaunchPlan& p) {
    p = launch_plan(a.m.kind, a.sa.kind, a.s.d, a.s.C, a.s.scale_uniform != 0, op);
    if (p.built && (p.k.map >= MAP_WPC) == wave)
        for (const UnitRow& r : rows)
            if (r.kind == a.m.kind) {
                UnitFn* f = op == OP_STEP && a.sa.kind == SK_RAM ? r.ram : r.unit;
                if (f) return f();
            }
    return KernelUnit{nullptr, nullptr, nullptr};
}

// ------------------------------------------------------------------ the dispatcher
// A runtime integer from the fixed list Vs, or a bool, as an integral_constant handed to a generic lambda; an integer
// outside the list is refused.  The lists are what bounds the set of instantiated kernels.
template <int... Vs, class F>
static hipError_t for_int(int v, F f) {
    hipError_t e = hipErrorInvalidValue;
    (void)(... || (v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)));   // instantiates in list order
    return e;
}
template <class F>
static hipError_t for_bool(bool v, F f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
template <class F>
static hipError_t for_bools(bool u, bool v, bool w, F f) {
    return for_bool(u, [&](auto a) {
        return for_bool(v, [&](auto b) { return for_bool(w, [&](auto c) { return f(a, b, c); }); });
    });
}

// Launch `kern`, whose template arguments and block size `k` restates, with the plan's grid -- when `k` is the instance
// the plan names: a dispatch that reached another instance fails rather than run a kernel that computes the same bits
// more slowly under a name it does not have.
template <class... P, class... A>
static hipError_t launch_inst(const LaunchPlan& p, const KernelInstance& k, void (*kern)(P...), hipStream_t st,
                                  const A&... args) {
    if (!p.built || !(p.k == k)) return hipErrorInvalidValue;
    kern<<<dim3((unsigned)p.grid), k.threads, 0, st>>>(args...);
    return hipGetLastError();
}

// A step launcher's result: the plan's instance is noted (mcmc_chains_step_kernel reports its name) once the dispatcher
// has accepted and launched it, so a refused launch leaves no name behind.
static inline hipError_t note_launched(hipError_t e, const LaunchPlan& p, const char* model) {
    if (e == hipSuccess) mcmc_note_step_instance(p.k, model);
    return e;
}

// what every unit states of its model class M and its row MK of kPlanModels
template <class M, int32_t MK>
constexpr PlanModel unit_model() {
    static_assert(plan_same_name(M::kName, plan_model(MK)->name), "the unit's model class is not its row's");
    return *plan_model(MK);
}

}  // namespace mcmc
