// tests/hostcheck/ntt_grid.h — TEST-ONLY: the fixed grid of Fr NTT planner inputs behind tests/golden/ntt_plans.txt and the line format of that
// file.  ntt_plancheck.cpp walks it over csrc/ntt_plan.h; the golden file was recorded by walking the same grid over the text of ntt_run as it
// stood inside ntt.hip before the planner became a header, its launches, reserves and table fetches replaced by calls of these print functions
// (profiles/scalar_drivers.md).  Nothing here knows a plan's layout.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

constexpr int NTT_GRID_CASES = 28 * 2 * 3 * 2 * 2;

// f(log_n, inverse, tile_env, cus, tw_arrays): every size, both directions, no tile override / one tile size everywhere, a device with more CUs
// than a small transform has tiles and one with fewer, the per-element twiddle arrays granted or refused (no memory: the kernel looks them up)
template <class F> void ntt_grid(F&& f) {
    for (int log_n = 1; log_n <= 28; ++log_n)
        for (int inverse = 0; inverse < 2; ++inverse)
            for (int tile_env : {0, 10, 11})
                for (int cus : {256, 8})
                    for (int tw_arrays = 1; tw_arrays >= 0; --tw_arrays) f(log_n, inverse != 0, tile_env, cus, tw_arrays != 0);
}

// The file is written without repetition: a plan is one line `#<i> ...`, written once, and one `ntt` line per (log_n, inverse) names the plan of its
// twelve cases as `tile_env/cus/arrays=#<i>`.
struct NttTable {
    std::vector<std::string> seen;     // the plans printed so far
    std::string plan, label, group_key, group, defs;
};
inline NttTable& ntt_table() { static NttTable t; return t; }
inline void ntt_flush_group() {
    NttTable& t = ntt_table();
    if (!t.group.empty()) printf("%s%s ->%s\n", t.defs.c_str(), t.group_key.c_str(), t.group.c_str());
    t.group.clear(); t.defs.clear();
}

inline void ntt_print_case(int log_n, bool inverse, int tile_env, int cus, bool tw_arrays) {
    NttTable& t = ntt_table();
    char buf[96];
    snprintf(buf, sizeof buf, "ntt log_n=%d inverse=%d", log_n, (int)inverse);
    if (t.group_key != buf) { ntt_flush_group(); t.group_key = buf; }
    snprintf(buf, sizeof buf, "%d/%d/%d", tile_env, cus, (int)tw_arrays);
    t.label = buf;
}
// the transform: the one instantiation of k_ntt_pass with its workgroup size, the passes, the bytes reserved in ws.data / ws.tmp (0: no reserve)
inline void ntt_print_plan(int tile_log, int kmax_t, int threads, int passes, size_t bytes_data, size_t bytes_tmp) {
    char buf[160];
    snprintf(buf, sizeof buf, "k_ntt_pass<%d,%d> threads=%d passes=%d data=%zu tmp=%zu", tile_log, kmax_t, threads, passes, bytes_data, bytes_tmp);
    ntt_table().plan = buf;
}
// one pass: the NttPassArgs its launch received (next = next_K / next_log_s, tiles = n_tiles), the grid, the buffers (caller / data / tmp), the twiddle array asked for (- none, plain, scaled =
// carrying 1/n) and whether the launch received one
inline void ntt_print_pass(int K, int log_s, int next_K, int next_log_s, int scale_log_n, uint32_t n_tiles, uint32_t grid, const char* src, const char* dst,
                           const char* tw_asked, bool tw_given) {
    char buf[200];
    snprintf(buf, sizeof buf, " | K=%d log_s=%d next=%d/%d scale=%d tiles=%u grid=%u %s->%s tw=%s%s", K, log_s, next_K, next_log_s, scale_log_n, n_tiles, grid,
             src, dst, tw_asked, tw_asked[0] == '-' ? "" : tw_given ? ":given" : ":refused");
    ntt_table().plan += buf;
}
// after the last pass of a case
inline void ntt_end_case() {
    NttTable& t = ntt_table();
    size_t id = 0;
    while (id < t.seen.size() && t.seen[id] != t.plan) ++id;
    if (id == t.seen.size()) { t.seen.push_back(t.plan); t.defs += "#" + std::to_string(id) + " " + t.plan + "\n"; }
    t.group += " " + t.label + "=#" + std::to_string(id);
}
// after the last case
inline void ntt_end_table() { ntt_flush_group(); }
