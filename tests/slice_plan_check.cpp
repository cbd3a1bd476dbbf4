// slice_plan_check.cpp -- walks launch_plan(..., OP_SLICE) (csrc/kernels/launch_plan.hpp) on the CPU: every family
// model, d = 1 .. 40 and the chain counts of launch_plan_check.cpp's walk.  It checks the instance names, that the grid
// covers the chains exactly, the block sizes, and the refusals (d > 32, the joint models past their catalogue sizes, the
// regression kinds, kind 10), and prints one line per plan:
//     slice <model> <d> <C> <built> <grid> <threads> <chains per block> <name>
// Built with -fsanitize=address,undefined by tests/test_slice_cpu.py.  Plain C++: no HIP runtime.
#define __host__
#define __device__
#include "../mcmc.jl_amd/csrc/kernels/launch_plan.hpp"

#include <string.h>

#include <initializer_list>

using namespace mcmc;

static int fails = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            fprintf(stderr, __VA_ARGS__);  \
            fprintf(stderr, "\n");         \
            ++fails;                       \
        }                                  \
    } while (0)

int main() {
    const int64_t Cs[] = {1, 2, 64, 65, 127, 128, 129, 1 << 20};
    int n = 0, built = 0;
    for (const PlanModel& pm : kPlanModels)
        for (int d = 1; d <= 40; ++d)
            for (int64_t C : Cs) {
                // the sampler argument is not read: any value plans the same
                const LaunchPlan p = launch_plan(pm.kind, SK_RWM, d, C, false, OP_SLICE);
                const LaunchPlan q = launch_plan(pm.kind, 0, d, C, true, OP_SLICE);
                CHECK(p.built == q.built && (!p.built || (p.k == q.k && p.grid == q.grid)), "%s d=%d: sampler read",
                      pm.name, d);
                const int nb = (d + 3) / 4;
                const bool want = d <= kSliceMaxD && nb <= pm.nuts_max_nb;
                CHECK(p.built == want, "%s d=%d C=%lld: built %d, want %d", pm.name, d, (long long)C, p.built, want);
                char name[96] = "-";
                if (p.built) {
                    ++built;
                    plan_kernel_name(name, sizeof name, p.k, pm.name);
                    char exp[96];
                    if (d <= kLaneMaxD) snprintf(exp, sizeof exp, "lpc_slice<%d, %s>", nb, pm.name);
                    else snprintf(exp, sizeof exp, "lpp_slice<%d, %s>", (nb + 1) / 2, pm.name);
                    CHECK(strcmp(name, exp) == 0, "%s d=%d: name %s, want %s", pm.name, d, name, exp);
                    CHECK(p.k.body == B_SLICE && p.k.map == (d <= kLaneMaxD ? MAP_LPC : MAP_LPP), "%s d=%d: family",
                          pm.name, d);
                    CHECK(p.k.threads == kPlanBlock, "%s d=%d: %d threads", pm.name, d, p.k.threads);
                    CHECK(p.chains_per_block == (d <= kLaneMaxD ? kPlanBlock : kPlanBlock / 2), "%s d=%d: %d chains",
                          pm.name, d, p.chains_per_block);
                    CHECK(p.grid * p.chains_per_block >= C && (p.grid - 1) * p.chains_per_block < C,
                          "%s d=%d C=%lld: grid %lld", pm.name, d, (long long)C, (long long)p.grid);
                    CHECK(!p.k.F && !p.k.US && !p.k.DA, "%s d=%d: flags", pm.name, d);
                }
                printf("slice %s %d %lld %d %lld %d %d %s\n", pm.name, d, (long long)C, p.built ? 1 : 0,
                       (long long)p.grid, p.k.threads, p.chains_per_block, name);
                ++n;
            }
    int outside = 0;
    for (int32_t kind : {0, (int32_t)MK_LOGISTIC, (int32_t)MK_LINEAR, (int32_t)MK_PROBIT, 10, -1})
        for (int d = 1; d <= 40; ++d) outside += launch_plan(kind, 0, d, 65, false, OP_SLICE).built;
    CHECK(outside == 0, "%d plans built outside the family", outside);
    CHECK(!launch_plan(MK_ISO, 0, 0, 65, false, OP_SLICE).built, "d = 0 built");
    printf("%d slice plans, %d built\n%d plans built outside the family\n", n, built, outside);
    return fails ? 1 : 0;
}
