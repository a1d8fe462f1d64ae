// tests/hostcheck/g1fft_grid.h — TEST-ONLY: the fixed grid of G1 FFT planner inputs behind tests/golden/g1fft_plans.txt and the line format of
// that file.  g1fft_plancheck.cpp walks it over csrc/g1fft_plan.h; the golden file was recorded by walking the same grid over the driver text
// of the commit before g1fft_plan.h existed, its launches and reserves replaced by calls of these print functions (profiles/g1fft_driver.md).
// Nothing here knows a plan's layout.  The file is written without repetition: a plan that an earlier case already had is named by its number only
// (most SRS shapes share their plans from 2^12 points on), a field that does not apply to a stage is left out, and consecutive in-place stages
// that differ only in their stage number are one line `log_s=first..last` (the radix-2 butterflies).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct G1fftSrsCase {
    const char* name;
    size_t srs_n;                  // 0: as long as the transform, at least 2^15 points
    bool lagrange, bits;
    int small_c, small_W, pre_c, pre_W;
    int max_log;
};

// ifft(case, log_n) for every SRS shape and size, then planes(log_n, inverse, scaled, strided), in the order of the golden file
template <class I, class P> void g1fft_grid(I&& ifft, P&& planes) {
    // window tables as srs.hip builds them: W = ceil(255 / c); c = 17 with the narrow c = 15 set beside it, or without it (it did not fit)
    const G1fftSrsCase shapes[] = {
        {"points", 0, false, false, 0, 0, 0, 0, 24},          {"points+bits", 0, false, true, 0, 0, 0, 0, 24},
        {"c13", 0, false, false, 0, 0, 13, 20, 24},           {"c13+bits", 0, false, true, 0, 0, 13, 20, 24},
        {"c15", 0, false, false, 0, 0, 15, 17, 24},           {"c15+bits", 0, false, true, 0, 0, 15, 17, 24},
        {"c15+narrow", 0, false, false, 15, 17, 15, 17, 24},  {"c15+narrow+bits", 0, false, true, 15, 17, 15, 17, 24},
        {"c17", 0, false, false, 0, 0, 17, 15, 24},           {"c17+bits", 0, false, true, 0, 0, 17, 15, 24},
        {"c17+narrow", 0, false, false, 15, 17, 17, 15, 24},  {"c17+narrow+bits", 0, false, true, 15, 17, 17, 15, 24},
        {"lagrange", 0, true, true, 15, 17, 17, 15, 24},      // a Lagrange handle that has tables: none of them may be used
        {"short", 1024, false, true, 0, 0, 13, 20, 10},       // fewer than 2 048 points with per-bit tables: the x3 tables cover the SRS
    };
    for (const G1fftSrsCase& s : shapes)
        for (int log_n = 0; log_n <= s.max_log; ++log_n) ifft(s, log_n);
    for (int log_n = 0; log_n <= 20; ++log_n)
        for (int inverse = 0; inverse < 2; ++inverse)
            for (int scaled = 0; scaled < 2; ++scaled)
                for (int strided = 0; strided < 2; ++strided) planes(log_n, inverse != 0, scaled != 0, strided != 0);
}
inline size_t g1fft_case_srs_n(const G1fftSrsCase& s, int log_n) {
    const size_t n = (size_t)1 << log_n;
    return s.srs_n ? s.srs_n : (n > 32768 ? n : 32768);
}

struct G1fftStageLine {
    std::string kernel, src, dst;
    size_t grid, sum_grid;
    int K, log_s, bitrev, last, scal;
    unsigned Q, wpo, partials;
    bool same_but_log_s(const G1fftStageLine& o) const {
        return kernel == o.kernel && src == o.src && dst == o.dst && grid == o.grid && sum_grid == o.sum_grid && K == o.K && bitrev == o.bitrev && last == o.last &&
               scal == o.scal && Q == o.Q && wpo == o.wpo && partials == o.partials;
    }
};
struct G1fftTable {
    std::vector<std::string> seen;     // the plans printed so far
    std::string plan;                  // the case being printed
    std::vector<G1fftStageLine> stages;
};
inline G1fftTable& g1fft_table() { static G1fftTable t; return t; }

inline void g1fft_print_ifft_case(const G1fftSrsCase& s, int log_n) { printf("ifft %s srs_n=%zu log_n=%d ->", s.name, g1fft_case_srs_n(s, log_n), log_n); }
inline void g1fft_print_planes_case(int log_n, bool inverse, bool scaled, bool strided) {
    printf("planes log_n=%d inverse=%d scaled=%d strided=%d ->", log_n, (int)inverse, (int)scaled, (int)strided);
}
// the form of a transform, read off the kernels it launches
inline const char* g1fft_form_of(bool bits, bool quads, bool first_tables, bool direct, bool radix2) {
    return bits ? (quads ? "bits+quads" : "bits") : first_tables ? "tables+direct" : direct ? "direct" : radix2 ? "radix2" : "copy";
}
// the plan: its form, workspace bytes, the buffer holding the result, the tables fetched (scalar-table keys in order, digit lists 1 of w^-e /
// 2 of w^-e / n with the points covered by the x3 tables, the window tables of a first-tables stage)
inline void g1fft_print_plan(const char* form, int stages, size_t a, size_t b, size_t c, const char* result, const int* keys, int n_keys, int naf, unsigned t3_points,
                             const char* tab, int tab_c, int tab_W) {
    char buf[256];
    std::string& out = g1fft_table().plan;
    snprintf(buf, sizeof buf, " form=%s stages=%d a=%zu b=%zu c=%zu result=%s scal=", form, stages, a, b, c, result);
    out = buf;
    for (int i = 0; i < n_keys; ++i) { snprintf(buf, sizeof buf, "%s%d", i ? "," : "", keys[i]); out += buf; }
    if (!n_keys) out += "-";
    if (naf || t3_points) { snprintf(buf, sizeof buf, " naf=%d t3_points=%u", naf, t3_points); out += buf; }
    if (tab_W) { snprintf(buf, sizeof buf, " tab=%s c=%d W=%d", tab, tab_c, tab_W); out += buf; }
    out += "\n";
}
// one stage: the kernel and what it is launched with; partials > 0: followed by k_g1fft_sum_partials on sum_grid workgroups
inline void g1fft_print_stage(const char* kernel, size_t grid, int K, int log_s, int bitrev, int last, int scal, unsigned Q, unsigned wpo, unsigned partials,
                              size_t sum_grid, const char* src, const char* dst) {
    g1fft_table().stages.push_back(G1fftStageLine{kernel, src, dst, grid, sum_grid, K, log_s, bitrev, last, scal, Q, wpo, partials});
}
// after the last stage of a case
inline void g1fft_end_case() {
    G1fftTable& t = g1fft_table();
    char buf[256];
    for (size_t i = 0; i < t.stages.size(); ++i) {
        const G1fftStageLine& s = t.stages[i];
        size_t j = i;
        while (s.src == s.dst && j + 1 < t.stages.size() && s.same_but_log_s(t.stages[j + 1]) && t.stages[j + 1].log_s == t.stages[j].log_s + 1) ++j;
        snprintf(buf, sizeof buf, "    %s grid=%zu K=%d log_s=%d", s.kernel.c_str(), s.grid, s.K, s.log_s);
        t.plan += buf;
        if (j > i) { snprintf(buf, sizeof buf, "..%d", t.stages[j].log_s); t.plan += buf; }
        if (s.bitrev) { snprintf(buf, sizeof buf, " bitrev=%d", s.bitrev); t.plan += buf; }
        snprintf(buf, sizeof buf, " last=%d scal=%d", s.last, s.scal);
        t.plan += buf;
        if (s.Q) { snprintf(buf, sizeof buf, " Q=%u", s.Q); t.plan += buf; }
        if (s.wpo) { snprintf(buf, sizeof buf, " wpo=%u", s.wpo); t.plan += buf; }
        if (s.partials) { snprintf(buf, sizeof buf, " partials=%u sum_grid=%zu", s.partials, s.sum_grid); t.plan += buf; }
        t.plan += " " + s.src + "->" + s.dst + "\n";
        i = j;
    }
    t.stages.clear();
    size_t id = 0;
    while (id < t.seen.size() && t.seen[id] != t.plan) ++id;
    if (id < t.seen.size()) { printf(" #%zu\n", id); return; }
    t.seen.push_back(t.plan);
    printf(" #%zu%s", id, t.plan.c_str());
}
