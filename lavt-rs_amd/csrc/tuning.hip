// Dispatch switches of liblavt_hip.  The LAVT_* environment variables below are read ONCE, at the first launch that asks (or again when the
// host calls lavt_tuning_reload(), which the test-suite does after changing one): no launch path calls getenv.  Every switch selects between
// kernels that compute the same result; none makes a kernel do less work.
#include <atomic>
#include <mutex>
#include <stdlib.h>

#include "common.h"

namespace {
lavt_tuning_t g_tuning;
std::atomic<bool> g_ready{false};
std::mutex g_mu;

int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
bool env_is(const char* name, char c) {
    const char* e = getenv(name);
    return e && e[0] == c;
}

void read_tuning(lavt_tuning_t& t) {
    t.gemm_tile = env_int("LAVT_GEMM_TILE", 0);                  // 64 | 128 | 512: forced tile configuration (tests exercise them)
    t.gemm_stages = env_int("LAVT_GEMM_STAGES", 0);              // 2 | 4: forced ring depth of the NT kernels (0: the dispatch rule)
    t.gemm_pipe = env_int("LAVT_GEMM_PIPE", 2);                  // gemm_nt_pipe.hip: 0 off, 1 the 256x256 tile, 2 + 128x128 tiles with K >= 1024, 3 + every 128x128 problem
    t.tn_pipe = env_int("LAVT_TN_PIPE", 2);                      // gemm_tn_pipe.hip: grouped weight gradients on 128x128 pipelined tiles -- 0: never (gemm_tn_v2.hip's 64x64 launch), 1: uncut groups only, 2: + long reductions cut into K pieces
    t.tn_pipe_min_tiles = env_int("LAVT_TN_PIPE_MIN_TILES", 128);
    t.tn_pipe_min_ktiles = env_int("LAVT_TN_PIPE_MIN_KTILES", 12);   // uncut groups: average K tiles per output tile below which the group stays on the 64x64 launch
    t.tn_pipe_stages = env_int("LAVT_TN_PIPE_STAGES", 4);        // 3 | 4
    t.bilinear_rows = !env_is("LAVT_BILINEAR_ROWS", '0');        // 0: the element-indexed bilinear forward instead of the row-staged one (the tests compare the two)
}
}  // namespace

const lavt_tuning_t& lavt_tuning() {
    if (!g_ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lk(g_mu);
        if (!g_ready.load(std::memory_order_relaxed)) {
            read_tuning(g_tuning);
            g_ready.store(true, std::memory_order_release);
        }
    }
    return g_tuning;
}

extern "C" int lavt_tuning_reload(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    read_tuning(g_tuning);
    g_ready.store(true, std::memory_order_release);
    return LAVT_OK;
}
