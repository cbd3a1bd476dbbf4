// state_table_check.cpp -- walks the host runtime's sampler table and chain-state table (csrc/host/tables.hpp) on
// the CPU: every kind x layout x tuner at d in {1, 16, 17, 40, 200} and C in {1, 65}.  Built by
// tests/test_state_table_cpu.py with -fsanitize=address,undefined; exits 0 when every check holds.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#define __host__
#define __device__
#include "../mcmc.jl_amd/csrc/host/tables.hpp"

using namespace mcmc;

static int g_bad = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            ++g_bad;                         \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");               \
        }                                    \
    } while (0)

int main() {
    // the tables themselves: every kind once, every ChainState pointer once
    std::set<int32_t> kinds;
    for (const SamplerInfo& si : kSamplers) {
        CHECK(kinds.insert(si.kind).second, "sampler kind %d has two rows", si.kind);
        CHECK(sampler_row(si.kind) == &si, "sampler_row(%d)", si.kind);
        CHECK(!si.lmc || si.rm_family, "%s: lmc outside rm_family", si.name);
        CHECK(!(si.records_leaps && si.leaps_refusal), "%s: records leaps and refuses them", si.name);
    }
    CHECK(kinds.size() == 11 && *kinds.begin() == SK_RWM && *kinds.rbegin() == SK_RMLMC, "sampler rows");
    CHECK(sampler_row(0) == nullptr && sampler_row(12) == nullptr, "unknown kinds have no row");
    std::set<std::string> names;
    size_t nbufs = 0;
    for (const StateBuf& b : kStateTable) {
        ++nbufs;
        CHECK(names.insert(b.name).second, "state buffer %s has two rows", b.name);
        CHECK((b.f64 != nullptr) != (b.i32 != nullptr), "%s: exactly one member pointer", b.name);
        CHECK((b.shape == SHAPE_I32) == (b.i32 != nullptr), "%s: shape and element type", b.name);
    }
    // ChainState is its device pointers and RAM's two strides: a member added without a row fails here
    CHECK(sizeof(ChainState) == nbufs * sizeof(void*) + 2 * sizeof(int64_t), "ChainState has a member without a row");
    ChainState probe;
    std::memset(&probe, 0, sizeof probe);
    for (const StateBuf& b : kStateTable) state_set(probe, b, (void*)&probe);
    probe.ram_ld = probe.ram_hs = -1;
    for (size_t i = 0; i < sizeof probe / sizeof(void*); ++i) {
        void* w;
        std::memcpy(&w, (const char*)&probe + i * sizeof(void*), sizeof w);
        CHECK(w != nullptr, "ChainState word %zu is reached by no row", i);
    }
    const std::set<std::string> dead_expected = {"sm_pG", "sm_pinvG", "nuts_wv", "nuts_ws", "mom"};

    const int ds[] = {1, 16, 17, 40, 200};
    const int64_t Cs[] = {1, 65};
    long ncfg = 0;
    for (const SamplerInfo& si : kSamplers)
        for (int layout = LAYOUT_LPC; layout <= LAYOUT_GLM; ++layout)
            for (int tuner = 0; tuner <= 1; ++tuner)
                for (int d : ds)
                    for (int64_t C : Cs) {
                        const Layout L = (Layout)layout;
                        const int64_t ld = L == LAYOUT_WPC ? round_up(d, 4) : round_up(C, 64);
                        const int d_pad = (int)round_up(d, 16);
                        const int64_t ram_hs = (int64_t)(packed_rows((int)round_up(d, 4)) + 1) * round_up(C, 256);
                        const StateDims dims{&si, tuner, L, d, C, ld, d_pad, 10, ram_hs};
                        ++ncfg;
                        // what create allocates, what fork copies, what free releases: the runtime's three walks
                        std::set<std::string> allocated, forked, freed;
                        for (const StateBuf& b : kStateTable) {
                            freed.insert(b.name);
                            if (!b.exists(dims)) continue;
                            allocated.insert(b.name);
                            const size_t n = state_count(b, dims);
                            CHECK(n > 0, "%s %s: empty", si.name, b.name);
                            CHECK(n * state_elem_bytes(b) / state_elem_bytes(b) == n, "%s %s: size overflow", si.name, b.name);
                            if (b.shape == SHAPE_STATE || b.shape == SHAPE_PACKED || b.shape == SHAPE_MOM)
                                CHECK(n % (size_t)ld == 0 && n / (size_t)ld >= 1, "%s %s: not whole rows", si.name, b.name);
                            if (b.shape == SHAPE_F64 || b.shape == SHAPE_I32)
                                CHECK(n >= (size_t)C && n % 64 == 0, "%s %s: per-chain padding", si.name, b.name);
                            if (b.live) forked.insert(b.name);
                        }
                        for (const std::string& n : forked)
                            CHECK(allocated.count(n), "%s: %s is forked but not allocated", si.name, n.c_str());
                        for (const std::string& n : allocated) {
                            CHECK(forked.count(n) || dead_expected.count(n),
                                  "%s: %s is allocated, not forked and not dead between steps", si.name, n.c_str());
                            CHECK(!(forked.count(n) && dead_expected.count(n)), "%s: %s is dead and forked", si.name,
                                  n.c_str());
                            CHECK(freed.count(n), "%s: %s is allocated but never freed", si.name, n.c_str());
                        }
                        // the state every sampler keeps, and the tuner state the sampler table names
                        CHECK(allocated.count("x") && allocated.count("lp"), "%s: x and lp", si.name);
                        const bool tuned_on = tuner && (si.tuner_state == TUNE_DRIFT || si.tuner_state == TUNE_LEAP);
                        CHECK(allocated.count("t_acc") == tuned_on && allocated.count("t_prop") == tuned_on,
                              "%s tuner %d: counters", si.name, tuner);
                        CHECK(allocated.count("t_leaps") == (tuner && si.tuner_state == TUNE_LEAP), "%s: t_leaps", si.name);
                        CHECK(allocated.count("t_step") == (tuned_on || si.tuner_state == TUNE_DUAL), "%s: t_step", si.name);
                        CHECK(allocated.count("t_bar") == (si.tuner_state == TUNE_DUAL), "%s: t_bar", si.name);
                        CHECK(allocated.count("ram_L") == (si.kind == SK_RAM), "%s: ram_L", si.name);
                        CHECK(allocated.count("sm_G") == si.manifold, "%s: sm_G", si.name);
                    }
    std::printf("%ld configurations, %d failures\n", ncfg, g_bad);
    return g_bad ? 1 : 0;
}
