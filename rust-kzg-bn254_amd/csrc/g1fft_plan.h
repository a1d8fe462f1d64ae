// g1fft_plan.h — the planner of the G1 FFT driver (g1fft.hip): from the length and the SRS's shape (g1_ifft), or the length and the direction
// (g1_fft_planes), to everything the driver decides before its first launch -- the form of the transform, its stages with their grids and scalar
// tables, the tables to fetch, the workspace bytes and the buffer that ends up holding the result.  Pure host code: no HIP type, no kzg_ctx,
// no allocation; also compiled with g++ by tests/hostcheck/g1fft_plancheck.cpp, which pins every plan of a fixed grid
// (tests/golden/g1fft_plans.txt).  The comments that quote measurements are the record of why a threshold has its value.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "host_log2.h"

namespace kzg {

constexpr uint32_t G1FFT_T3_MAX = 2048;                  // the x3 tables cover the first min(SRS length, 2048) points: every point the table paths transform
constexpr size_t G1FFT_POINT_BYTES = 36 * 4;             // one XYZZ value in limb planes (4 coordinates of NL = 9 limbs)

// The part of an SRS the planner reads (kzg_srs, engine.h)
struct G1fftSrsShape {
    size_t n = 0;                  // SRS length
    bool monomial = true;          // lagrange_of == 0: the table paths hold multiples of the points this handle transforms
    bool bit_tables = false;       // per-bit tables Bit_p[j] = 2^p P_j exist
    int small_c = 0, small_W = 0;  // the narrow window-table set, or zero
    int pre_c = 0, pre_W = 0;      // the window tables of the SRS's MSMs, or zero
};

enum G1fftForm {
    G1FFT_COPY,                    // one point: no stage
    G1FFT_BITS_WHOLE,              // the whole transform through the per-bit tables
    G1FFT_BITS_QUADS,              // first stage through the per-bit tables, then direct stages on lane quads
    G1FFT_TABLES_DIRECT,           // first stage through the SRS window tables, then direct stages
    G1FFT_DIRECT,                  // direct stages on lanes or pairs
    G1FFT_RADIX2,                  // radix-2 butterflies on lanes or pairs
    G1FFT_FORMS
};
enum G1fftStageKind {
    G1S_LOAD, G1S_LOAD_BITREV,     // k_g1fft_load: SRS points -> planes
    G1S_GATHER, G1S_GATHER_BITREV, // k_g1fft_gather_planes: planes of another stride -> planes
    G1S_BITS,                      // k_g1fft_bits
    G1S_FIRST_TABLES,              // k_g1fft_first_tables
    G1S_DIRECT, G1S_DIRECT_PAIRS,  // k_g1fft_direct, k_g1fft_direct_pairs
    G1S_MUL_QUADS,                 // k_g1fft_mul_quads
    G1S_RADIX2, G1S_RADIX2_PAIRS,  // k_g1fft_stage, k_g1fft_stage_pairs
    G1S_GATHER_PAD,                // k_g1fft_pad_planes: the first `nonzero` points of the input, the identity after them (host_encode.h)
    G1S_SPREAD_BITREV,             // k_g1fft_spread_planes: the bit-reversed load and the first log_s radix-2 stages of a zero-padded input
    G1S_KINDS
};
// the key of a scalar table (get_scalars): bit 0 = times 1/n, bits 1-2 = canon (1: canonical integers), bit 3 = forward (w^+e)
enum { G1SCAL_SCALED = 1, G1SCAL_CANON = 2, G1SCAL_FORWARD = 8, G1SCAL_KEYS = 16 };
enum { G1BUF_INPUT = -1 };         // a stage's source: the transform's input (SRS points or tables, the caller's planes), else plane buffer 0 or 1

struct G1fftStage {
    G1fftStageKind kind;
    int K;                         // radix bits (0: load / gather)
    int log_s;                     // log2 of the stride of a direct stage after the first; the stage number s of a radix-2 stage
    bool last;                     // the `last` flag of a direct or radix-2 kernel: every term is multiplied (1/n folded into the scalars)
    size_t grid;                   // workgroups of 256 lanes
    uint32_t Q, wpo;               // bits stage: slices per term; bits / first-tables stage: waves per output
    int scal;                      // the scalar table the kernel reads (get_scalars key), -1: none (a bits stage reads the digit lists)
    uint32_t partials;             // > 0: the stage writes that many partial sums per output and k_g1fft_sum_partials adds them into dst
    int src, dst;                  // plane buffers (G1BUF_INPUT, 0, 1); radix-2 stages work in place
};

constexpr int G1FFT_MAX_STAGES = 36;   // a load and 32 radix-2 stages at most (n < 2^32)

struct G1fftPlan {
    uint32_t n;
    int log_n;
    G1fftForm form;
    int n_stages;
    G1fftStage stage[G1FFT_MAX_STAGES];
    size_t sum_grid;               // grid of k_g1fft_sum_partials: one wave per output
    int scal_keys[3], n_scal_keys; // the scalar tables to fetch, in the driver's order
    bool t3;                       // the x3 / x5 / x7 tables of the first t3_points SRS points are needed
    uint32_t t3_points;
    int naf;                       // the NAF digit lists: 0 none, 1 of w^-e, 2 of w^-e / n
    bool tab_small; int tab_c, tab_W;   // first-tables stage: the narrow set or the SRS's own, window bits, tables
    size_t bytes_a, bytes_b, bytes_c;   // workspaces poly[0].a (prefix products of the affine conversion), .b (two plane sets), .c (partial sums)
    int result;                    // the plane buffer (0 or 1) that holds the result
    uint32_t batch;                // transforms per launch (grid.y of the plane-to-plane stage kernels); the grids above are those of ONE transform
};

inline int g1fft_log2(size_t n) { return ilog2_ceil(n); }

// Stage plan.  A stage is one scalar multiplication deep whatever it computes, so the plan minimises (number of stages) x (time of a
// stage).  Measured stage times on MI355X (tools/time_g1ifft.py, round 3) while the stage fits ONE wave per SIMD (65536 lanes):
// 1.25 ms with one lane per point, 0.83 ms on lane pairs; beyond that a stage is throughput bound and scales with its lanes (a lone
// wave already issues most of what its SIMD can: two pair waves per SIMD took 1.44 ms).  Candidates:
//   direct stages of radix 2^K (one lane or pair per (output, term): n 2^K lanes or pairs), K <= 5
//   radix-2 butterflies (n / 2 lanes or pairs, work bound: one multiplication per two outputs)
// *kmax = 0: radix-2 butterflies; else the largest radix bits of the direct stages.  (Shared by g1_ifft and g1_fft_planes.)
// batch: that many transforms of n points share every launch (the blobs of a group of kzg_encode_cosets_batch, a grid dimension of the
// stage kernels): a stage's lanes are the lanes of one transform times the batch, so a radix that fills the chip for one transform
// overfills it for eight and the choice moves to smaller radices.  batch = 1 is the choice of a single transform, term for term.
// Measured on batched stages (profiles/encode_batch.md, one kernel trace per batch of 1, 16 and 64 blobs at d = 2^12, r = 8, l = 16): a stage
// of a batch that stays within one wave per SIMD takes what a single transform's stage takes -- 1.26 - 1.37 ms on lanes, 0.69 - 0.77 ms on
// pairs -- and a stage beyond it scales with its lanes (k_fk20_lincomb: 1.28 ms at 8 192 lanes, 2.80 ms at 131 072, 10.5 ms at 524 288), so the
// constants below serve batches as they stand; whole calls land within 6 % of the model's sum of stages.
inline void g1fft_choose_plan_batch(size_t n, int log_n, size_t batch, int* kmax_out, bool* pairs_out) {
    int kmax = 0;
    bool pairs = false;
    const double t_lane = 1.25, t_pair = 0.83, cap = 65536.0;
    double best = 1e300;
    for (int mode = 0; mode < 2; ++mode) {                        // 0: one lane per point, 1: lane pairs
        const double t1 = mode ? t_pair : t_lane, width = mode ? 2.0 : 1.0;
        for (int K = 2; K <= 5 && K <= std::max(log_n, 2); ++K) {  // direct stages
            const double lanes = (double)n * (double)(1u << K) * width * (double)batch;
            const double cost = (double)((log_n + K - 1) / K) * t1 * std::max(1.0, lanes / cap);
            if (cost < best) { best = cost; kmax = K; pairs = mode != 0; }
        }
        const double lanes2 = (double)n / 2.0 * width * (double)batch;             // radix-2 butterflies (+ the scaling multiplication of the last stage)
        const double cost2 = (double)(log_n + 1) * t1 * std::max(1.0, lanes2 / cap);
        if (cost2 < best) { best = cost2; kmax = 0; pairs = mode != 0; }
    }
    *kmax_out = kmax;
    *pairs_out = pairs;
}
inline void g1fft_choose_plan(size_t n, int log_n, int* kmax_out, bool* pairs_out) { g1fft_choose_plan_batch(n, log_n, 1, kmax_out, pairs_out); }

inline G1fftPlan g1fft_plan_begin(size_t n) {
    G1fftPlan p{};
    p.n = (uint32_t)n;
    p.log_n = g1fft_log2(n);
    p.sum_grid = (n * 64 + 255) / 256;
    p.batch = 1;
    return p;
}
inline G1fftStage& g1fft_push(G1fftPlan& p, G1fftStageKind kind, size_t lanes, int src, int dst) {
    G1fftStage& s = p.stage[p.n_stages++];
    s.kind = kind;
    s.grid = (lanes + 255) / 256;
    s.scal = -1;
    s.src = src;
    s.dst = dst;
    return s;
}

// The forms every transform can take: a copy (one point), direct stages of balanced radix bits (srs: the first one through the window
// tables where they pay), or radix-2 butterflies.  Buffer 0 takes the input copy; the direct stages alternate between the two buffers.
// copy_in: the input is not a plane set of stride n (SRS points, a slice of longer planes); scal_mid / scal_last: the scalar tables of
// the stages before the last and of the last, whose `last` flag is last_flag.
inline void g1fft_plan_stages(G1fftPlan& p, const G1fftSrsShape* srs, bool copy_in, int scal_mid, int scal_last, bool last_flag) {
    const size_t n = p.n;
    const int log_n = p.log_n;
    const G1fftStageKind copy = srs ? G1S_LOAD : G1S_GATHER, copy_bitrev = srs ? G1S_LOAD_BITREV : G1S_GATHER_BITREV;
    int kmax = 0;
    bool pairs = false;
    g1fft_choose_plan_batch(n, log_n, p.batch, &kmax, &pairs);
    if (log_n == 0) {
        p.form = G1FFT_COPY;
        g1fft_push(p, copy, n, G1BUF_INPUT, 0);
    } else if (kmax >= 2) {
        const int stages = (log_n + kmax - 1) / kmax;
        // the first stage through the SRS window tables when the SRS has them and the stage fits four waves per SIMD
        // Prefers the narrow (c = 15) set: fewer double-and-add steps per digit.
        if (srs && srs->monomial) {
            if (srs->small_W > 0) { p.tab_small = true; p.tab_c = srs->small_c; p.tab_W = srs->small_W; }
            else if (srs->pre_W > 0) { p.tab_c = srs->pre_c; p.tab_W = srs->pre_W; }
        }
        const int K0 = (log_n + stages - 1) / stages;                       // radix bits of the first stage (balanced split)
        const uint32_t wpo = p.tab_W ? (uint32_t)((((size_t)1 << K0) * p.tab_W + 31) / 32) : 0;
        const bool first_tables = p.tab_W && wpo <= 32 && n * (size_t)wpo <= 4096;
        if (!first_tables) { p.tab_small = false; p.tab_c = p.tab_W = 0; }
        p.form = first_tables ? G1FFT_TABLES_DIRECT : G1FFT_DIRECT;
        if (!first_tables && copy_in) g1fft_push(p, copy, n, G1BUF_INPUT, 0);
        int done = 0;
        for (int i = 0; i < stages; ++i) {
            const int K = (log_n - done + (stages - i) - 1) / (stages - i);   // balanced split of the remaining bits
            done += K;
            const bool last = i == stages - 1;
            const size_t lanes = n << K;
            const bool tables = i == 0 && first_tables;
            G1fftStage& s = tables ? g1fft_push(p, G1S_FIRST_TABLES, n * (size_t)wpo * 64, G1BUF_INPUT, 1)
                                   : g1fft_push(p, pairs ? G1S_DIRECT_PAIRS : G1S_DIRECT, pairs ? 2 * lanes : lanes, i == 0 && !copy_in ? G1BUF_INPUT : (i & 1), 1 - (i & 1));
            s.K = K;
            if (tables) {
                s.scal = G1SCAL_CANON | (last ? G1SCAL_SCALED : 0);          // canonical scalars (scaled by 1/n when this is also the last stage)
                s.wpo = s.partials = wpo;
                p.scal_keys[p.n_scal_keys++] = s.scal;
                p.bytes_c = n * wpo * G1FFT_POINT_BYTES;
            } else {
                s.log_s = log_n - done;
                s.last = last && last_flag;
                s.scal = last ? scal_last : scal_mid;
            }
        }
        p.result = stages & 1;
    } else {
        p.form = G1FFT_RADIX2;
        g1fft_push(p, copy_bitrev, n, G1BUF_INPUT, 0);
        for (int st = 1; st <= log_n; ++st) {
            const bool last = st == log_n;
            G1fftStage& s = g1fft_push(p, pairs ? G1S_RADIX2_PAIRS : G1S_RADIX2, pairs ? n : n / 2, 0, 0);
            s.K = 1;
            s.log_s = st;
            s.last = last && last_flag;
            s.scal = last ? scal_last : scal_mid;
        }
    }
}

// g1_ifft: the Lagrange basis of the first n points of an SRS.  The result is in plane buffer `result` of poly[0].b.
inline G1fftPlan g1fft_plan_ifft(size_t n, const G1fftSrsShape& srs) {
    G1fftPlan p = g1fft_plan_begin(n);
    const int log_n = p.log_n;
    p.bytes_b = n * G1FFT_POINT_BYTES * 2;                        // two XYZZ plane sets (ping-pong)
    p.bytes_a = n * G1FFT_POINT_BYTES / 4;                        // prefix products of the affine conversion
    p.scal_keys[p.n_scal_keys++] = 0;
    p.scal_keys[p.n_scal_keys++] = G1SCAL_SCALED;
    // 64 .. 256 points of an SRS with per-bit tables: the whole transform as sums of table points (k_g1fft_bits);
    // 512 .. 2048 points: the FIRST STAGE that way (radix 2^K0 over the SRS points: n 2^K0 x 64 mixed additions at the chip's throughput
    // instead of a 127-step scalar-multiplication chain), the rest as one or two direct stages on lane quads
    const bool by_bits = srs.bit_tables && srs.monomial;
    if (by_bits && n >= 64 && n <= 256) {
        p.form = G1FFT_BITS_WHOLE;
        // slices per term: two waves per SIMD in all (n^2 Q / 32 = 2048 waves) -- more waves only add tree additions (every wave ends in a
        // 5-level tree: a third of the work at 21 digits per pair), fewer leave lone waves at half the issue rate.  Measured: 256 points
        // 0.71 ms with Q = 4, 0.66 with Q = 1; 128 points 0.28 -> 0.26 (tools/time_g1ifft.py).  The floor is the additions themselves:
        // n^2 x 85 (5.6 M at 256 points = 0.36 ms of the chip).
        const uint32_t Q = (uint32_t)std::max<size_t>(1, 65536 / (n * n)), wpo = (uint32_t)(n * Q / 32);
        G1fftStage& s = g1fft_push(p, G1S_BITS, n * (size_t)wpo * 64, G1BUF_INPUT, 0);
        s.K = log_n;
        s.Q = Q;
        s.wpo = s.partials = wpo;
        p.naf = 2;
        p.bytes_c = (size_t)n * wpo * G1FFT_POINT_BYTES;
    } else if (by_bits && n >= 512 && n <= G1FFT_T3_MAX) {
        p.form = G1FFT_BITS_QUADS;
        // Plan (bits of the stages, first one through the per-bit tables): the later stages are one 127-step GLV chain deep each, pure latency
        // while they fit one wave per SIMD (65 536 lanes = 16 384 quads = n 2^K <= 16 384).  512 = 2^4 . 2^5, 1024 = 2^6 . 2^4, 2048 = 2^5 . 2^3 . 2^3
        // (measured against 5,4 / 3,3,3 / 5,5 / 4,3,3 / 6,5 / 7,4 and against the later stages on lane pairs: tools/time_g1ifft.py, profiles/r03d_quad.md).
        int plan[4] = {0, 0, 0, 0}, np = 0;
        if (log_n == 9) { plan[0] = 4; plan[1] = 5; np = 2; }
        else if (log_n == 10) { plan[0] = 6; plan[1] = 4; np = 2; }
        else { plan[0] = 5; plan[1] = 3; plan[2] = 3; np = 3; }
        const int K0 = plan[0];
        const size_t R0 = (size_t)1 << K0;
        const uint32_t Q = (uint32_t)std::max<size_t>(std::max<size_t>(1, 32 / R0), 65536 / (n * R0)), wpo = (uint32_t)(R0 * Q / 32);
        size_t part_points = (size_t)n * wpo;
        for (int i = 1; i < np; ++i) part_points = std::max(part_points, n << plan[i]);
        p.bytes_c = part_points * G1FFT_POINT_BYTES;
        p.naf = 1;
        G1fftStage& s0 = g1fft_push(p, G1S_BITS, n * (size_t)wpo * 64, G1BUF_INPUT, 1);
        s0.K = K0;
        s0.Q = Q;
        s0.wpo = s0.partials = wpo;
        int done = K0;
        for (int i = 1; i < np; ++i) {
            const int K = plan[i];
            done += K;
            const bool last = i == np - 1;
            G1fftStage& s = g1fft_push(p, G1S_MUL_QUADS, 4 * (n << K), i & 1, 1 - (i & 1));
            s.K = K;
            s.log_s = log_n - done;
            s.last = last;
            s.scal = last ? G1SCAL_SCALED : 0;
            s.partials = (uint32_t)1 << K;
        }
        p.result = np & 1;
    } else {
        g1fft_plan_stages(p, &srs, true, 0, G1SCAL_SCALED, true);
    }
    p.t3 = p.naf != 0;
    p.t3_points = p.t3 ? (uint32_t)std::min<size_t>(srs.n, G1FFT_T3_MAX) : 0;
    return p;
}

// g1_fft_planes: out = sum_j w^(+-ij) in[j] (times 1/n if scaled) on the caller's plane buffers; strided: in_stride != n.  No workspace.
// The caller names buffer `result` out and the other one tmp, so the transform ends in out.  batch: transforms per launch (plane sets a
// fixed distance apart, one per grid.y); the stage plan is chosen for batch x the lanes of one transform.
inline G1fftPlan g1fft_plan_planes(size_t n, bool inverse, bool scaled, bool strided, size_t batch = 1) {
    G1fftPlan p = g1fft_plan_begin(n);
    p.batch = (uint32_t)batch;
    const int dir = inverse ? 0 : G1SCAL_FORWARD;
    if (p.log_n > 0) {                                            // one point: the transform (and 1/1) is the identity
        p.scal_keys[p.n_scal_keys++] = dir;
        if (scaled) p.scal_keys[p.n_scal_keys++] = dir | G1SCAL_SCALED;
    }
    g1fft_plan_stages(p, nullptr, strided, dir, scaled ? dir | G1SCAL_SCALED : dir, scaled);   // the last stage multiplies every term (1/n folded in)
    return p;
}

}  // namespace kzg
