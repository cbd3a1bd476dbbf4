// launch_plan_check.cpp -- walks the launch plan of the separable and joint targets (csrc/kernels/launch_plan.hpp) on
// the CPU and prints what it names: every model kind of the family x RWM / MALA / HMC / HMCDA / RAM / NUTS x every d of
// 1 .. 40 and of the command line x C in {1, 2, 64, 65, 127, 128, 129, 2^20} x both scale kinds, one line each; then
// the eval, record and NUTS-init plans over the same models, widths and chain counts.  Built and run by
// tests/test_launch_plan_cpu.py with -fsanitize=address,undefined, which checks the lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#define __host__
#define __device__
#include "../mcmc.jl_amd/csrc/kernels/launch_plan.hpp"

using namespace mcmc;

static long g_lines = 0;

static void line(const char* op, const PlanModel& m, const char* sampler, int d, long long C, int us,
                 const LaunchPlan& p) {
    char name[160] = "-";                              // the library's buffer (context.cpp) is this long
    if (p.built && plan_kernel_name(name, sizeof name, p.k, m.name) >= (int)sizeof name) std::abort();
    // the name last: it holds blanks
    std::printf("%s %s %s %d %lld %d %d %lld %d %d %s\n", op, m.name, sampler, d, C, us, (int)p.built, (long long)p.grid,
                p.k.threads, p.chains_per_block, name);
    ++g_lines;
}

int main(int argc, char** argv) {
    std::set<int> ds;
    for (int d = 1; d <= 40; ++d) ds.insert(d);
    for (int i = 1; i < argc; ++i) ds.insert(std::atoi(argv[i]));
    const long long Cs[] = {1, 2, 64, 65, 127, 128, 129, 1ll << 20};
    const struct { int32_t kind; const char* name; } samplers[] = {{SK_RWM, "rwm"}, {SK_MALA, "mala"}, {SK_HMC, "hmc"},
                                                                  {SK_HMCDA, "hmcda"}, {SK_RAM, "ram"}, {SK_NUTS, "nuts"}};
    for (const PlanModel& m : kPlanModels)
        for (const auto& s : samplers)
            for (int d : ds)
                for (long long C : Cs)
                    for (int us = 0; us < 2; ++us)
                        line("step", m, s.name, d, C, us, launch_plan(m.kind, s.kind, d, C, us != 0, OP_STEP));
    std::printf("%ld combinations\n", g_lines);
    g_lines = 0;
    for (const PlanModel& m : kPlanModels)
        for (int d : ds)
            for (long long C : Cs) {
                line("eval", m, "-", d, C, 0, launch_plan(m.kind, SK_RWM, d, C, false, OP_EVAL));
                line("record", m, "hmc", d, C, 0, launch_plan(m.kind, SK_HMC, d, C, false, OP_RECORD));
                line("record", m, "hmcda", d, C, 0, launch_plan(m.kind, SK_HMCDA, d, C, false, OP_RECORD));
                line("init", m, "nuts", d, C, 0, launch_plan(m.kind, SK_NUTS, d, C, false, OP_NUTS_INIT));
            }
    std::printf("%ld further plans\n", g_lines);
    // outside the family and outside the widths: nothing is built
    int bad = 0;
    for (int32_t kind : {0, (int)MK_LOGISTIC, (int)MK_LINEAR, (int)MK_PROBIT, 10})
        for (const auto& s : samplers) bad += launch_plan(kind, s.kind, 3, 65, false, OP_STEP).built;
    for (const PlanModel& m : kPlanModels)
        for (int d : {-1, 0, kBlockMaxD + 1})
            for (const auto& s : samplers) bad += launch_plan(m.kind, s.kind, d, 65, false, OP_STEP).built;
    for (int32_t sk : {0, (int)SK_SMMALA, (int)SK_RMLMC}) bad += launch_plan(MK_ISO, sk, 3, 65, false, OP_STEP).built;
    std::printf("%d plans built outside the family\n", bad);
    return bad != 0;
}
