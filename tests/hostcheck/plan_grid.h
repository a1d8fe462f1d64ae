// tests/hostcheck/plan_grid.h — TEST-ONLY: the fixed grid of MSM planner inputs behind tests/golden/msm_plans.txt and the line format of that
// file.  plancheck.cpp walks it over csrc/msm_plan.h; the golden file was recorded by walking the same grid over the planner text of the
// commit before msm_plan.h existed (profiles/msm_driver.md).  Nothing here knows a plan's layout beyond its field names.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

struct GridCase {
    const char* bases;                 // name of the base set (printed)
    uint32_t stride; int c, W; bool naf, bitsum;                       // non-pointer part of the bases
    size_t n; uint32_t batch, polys;
    bool alone; int lanes, c_over, seg_over; uint32_t wave_slots;      // the context's part
    uint32_t out_off, out_cap;                                         // this launch's window of the result buffer
};

// run(GridCase) for every case, in the order of the golden file
template <class F> void plan_grid(F&& run) {
    constexpr size_t K14 = (size_t)1 << 14, K15 = (size_t)1 << 15, K18 = (size_t)1 << 18, K19 = (size_t)1 << 19, K20 = (size_t)1 << 20, K24 = (size_t)1 << 24;
    // every size threshold of the planner and its neighbour below
    const size_t ns[] = {1, 127, 128, 512, 513, 2048, 2049, 4096, 4097, 8192, 8193, K14 - 1, K14, K15 - 1, K15, K18 - 1, K18, K19 - 1, K19, K20, K20 + 1, K24};
    const uint32_t ALL = 16384;        // a whole result buffer (MSM_MAX_OUT)
    auto naf_c = [](size_t n) { return n < K15 ? 13 : n >= K20 ? 17 : n >= K18 ? 16 : 15; };      // (engine.h srs_naf_c)
    auto ctx = [&](GridCase g, bool alone, int lanes, int c_over, int seg_over) {
        g.alone = alone; g.lanes = lanes; g.c_over = c_over; g.seg_over = seg_over;
        run(g);
    };
    // generic mode (caller bases): batch 1 at every size, 3 and 64 at a few; the window override
    for (size_t n : ns) ctx({"generic", 0, 0, 0, false, false, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, 0);
    for (uint32_t batch : {3u, 64u})
        for (size_t n : {(size_t)1, (size_t)128, (size_t)4097, K14, K18}) ctx({"generic", 0, 0, 0, false, false, n, batch, 0, true, 0, 0, 0, 3072, 0, ALL}, batch == 3, 0, 0, 0);
    for (int c_over : {2, 16})
        for (size_t n : {(size_t)513, K15, K20}) ctx({"generic", 0, 0, 0, false, false, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, c_over, c_over == 2 ? 7 : 0);
    ctx({"generic", 0, 0, 0, false, false, 4096, 0, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, 0);                     // batch == 0
    ctx({"generic", 0, 0, 0, false, false, 128, 200, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 2, 0);                    // 128 windows x 200 MSMs: more window sums than the result buffer holds
    ctx({"generic", 0, 0, 0, false, false, 128, 64, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 16, 0);                    // 1024 sets of 2^15 buckets: the scan limit
    ctx({"generic", 0, 0, 0, false, false, 128, 64, 0, true, 0, 0, 0, 3072, 256, 256}, true, 0, 0, 0);                   // 64 x 64 window sums against a 256-point window
    ctx({"generic", 0, 0, 0, false, false, 128, 1, 2, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, 0);                      // polys without per-bit tables
    // window tables, c = 17 (15 tables), one SRS length apart: 2^20 (indices as they are) and 2^22 (compact indices, parts of 2^20)
    for (uint32_t stride : {(uint32_t)K20, (uint32_t)(4 * K20)})
        for (size_t n : ns) {
            if (n > K20) continue;
            const bool part = stride > K20 && n == K20;
            ctx({"tables17", stride, 17, 15, false, false, n, 1, 0, true, 0, 0, 0, 3072, part ? 3 * 256u : 0u, part ? 256u : ALL}, stride == K20 || n < K14, 0, 0, 0);
        }
    ctx({"tables17", (uint32_t)K20, 17, 15, false, false, K20, 3, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, 0);      // tables with batch > 1
    ctx({"tables17", (uint32_t)K20, 17, 15, false, false, K20, 1, 0, true, 0, 0, 0, 3072, ALL - 100, 256}, true, 0, 0, 0);   // 208 points past the end of the buffer
    ctx({"tables24", (uint32_t)K20, 24, 11, false, false, K20, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, 0);      // 2^23 buckets: the scan limit
    // the c = 15 set (17 tables) of MSMs up to 2^13 pairs: fused first level up to 2^11; lane pairs / quads; forced trip counts
    for (size_t n : ns) {
        if (n > 8193) continue;
        for (bool alone : {true, false}) ctx({"tables15", (uint32_t)K20, 15, 17, false, false, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, alone, 0, 0, 0);
    }
    for (int lanes : {2, 4})
        for (size_t n : {(size_t)512, (size_t)8192}) ctx({"tables15", (uint32_t)K20, 15, 17, false, false, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, lanes == 2, lanes, 0, 0);
    for (int seg : {1, 7}) ctx({"tables15", (uint32_t)K20, 15, 17, false, false, 4097, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, seg);
    // bit sums over the per-bit tables (what the kernels take: up to 2^13 pairs)
    for (size_t n : ns) {
        if (n > 8192) continue;
        ctx({"bitsum", (uint32_t)K15, 0, 255, false, true, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, n != 513, 0, 0, 0);
    }
    ctx({"bitsum", (uint32_t)K15, 0, 255, false, true, 8192, 1, 0, true, 0, 0, 0, 3072, 0, 8}, true, 0, 0, 0);          // 16 result points against a window of 8
    // NAF digits over the per-bit tables, bucket bits by length
    for (size_t n : ns) {
        if (n < 8193) continue;
        const uint32_t stride = (uint32_t)(n > K20 ? K24 : K20);
        for (bool alone : {true, false}) ctx({"naf", stride, naf_c(n), 255, true, false, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, alone, 0, 0, 0);
    }
    for (int lanes : {2, 4})
        for (size_t n : {K14, K18, K20}) ctx({"naf", (uint32_t)K20, naf_c(n), 255, true, false, n, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, lanes == 4, lanes, 0, 0);
    for (int seg : {1, 7}) ctx({"naf", (uint32_t)K20, naf_c(K15), 255, true, false, K15, 1, 0, true, 0, 0, 0, 3072, 0, ALL}, false, 0, 0, seg);
    // batched NAF: polynomials of one length over the same tables
    for (size_t len : {(size_t)64, (size_t)1 << 12, (size_t)1 << 13, K15, K18})
        for (uint32_t polys : {1u, 2u, 16u, 1024u, 1025u})
            ctx({"naf", (uint32_t)K20, naf_c(len), 255, true, false, len * polys, 1, polys, true, 0, 0, 0, 3072, 0, ALL}, polys != 2, 0, 0, 0);
    ctx({"naf", (uint32_t)K20, 13, 255, true, false, 64 * 3 + 1, 1, 3, true, 0, 0, 0, 3072, 0, ALL}, true, 0, 0, 0);    // length no multiple of polys
}

// launch_len(bases) and capacity(poly_len): the two size rules beside the plan
template <class L, class C> void plan_grid_sizes(L&& launch_len, C&& capacity) {
    struct { const char* name; uint32_t stride; int W; bool naf; } sets[] = {{"generic", 0, 0, false}, {"tables17", 1u << 20, 15, false}, {"tables17", 1u << 22, 15, false},
                                                                            {"tables17", 1u << 24, 15, false}, {"tables15", 1u << 20, 17, false}, {"naf", 1u << 24, 255, true}};
    for (auto& s : sets) printf("launch_len %s stride=%u W=%d -> %zu\n", s.name, s.stride, s.W, (size_t)launch_len(s.stride, s.W, s.naf));
    for (size_t len : {(size_t)0, (size_t)1, (size_t)64, (size_t)8191, (size_t)8192, (size_t)32767, (size_t)32768, (size_t)262143, (size_t)262144, (size_t)1 << 24, ((size_t)1 << 24) + 1})
        printf("batch_capacity len=%zu -> %zu\n", len, (size_t)capacity(len));
}

inline void print_case(const GridCase& g) {
    printf("%s stride=%u c=%d W=%d n=%zu batch=%u polys=%u alone=%d lanes=%d c_over=%d seg=%d slots=%u off=%u cap=%u ->", g.bases, g.stride, g.c, g.W, g.n, g.batch,
           g.polys, (int)g.alone, g.lanes, g.c_over, g.seg_over, g.wave_slots, g.out_off, g.out_cap);
}
// a rejected launch: the status and whether last_error gets a text of its own
inline void print_rejected(const GridCase& g, int status, const char* error) {
    print_case(g);
    printf(" status=%d%s%s\n", status, error ? " error=" : "", error ? error : "");
}
// an accepted launch: every field of the plan (P: any struct with these names), then what the driver derives from it
template <class P>
void print_plan(const GridCase& g, const P& p, bool fused, int ND, bool lean_sort, bool level1_quads, uint32_t n_out) {
    print_case(g);
    printf(" status=0 n=%u batch=%u tables=%d naf=%d polys=%u c=%d W=%d B=%u sets=%u G=%u nl=%u set_len=%u tile_len=%u tiles_per_set=%u tiles=%u bitsum=%d fused=%d quad=%d"
           " alone=%d sort2=%d sort_small=%d Hb=%u tile1=%u tiles1=%u tiles2cap=%u T=%u m=%u idx_stride=%u idx_log=%u stride_adj=%u | ND=%d lean=%d quad1=%d n_out=%u\n",
           p.n, p.batch, (int)p.tables, (int)p.naf, p.polys, p.c, p.W, p.B, p.sets, p.G, p.nl, p.set_len, p.tile_len, p.tiles_per_set, p.tiles, (int)p.bitsum, (int)fused,
           (int)p.quad, (int)p.alone, (int)p.sort2, (int)p.sort_small, p.Hb, p.tile1, p.tiles1, p.tiles2cap, p.T, p.m, p.idx_stride, p.idx_log, p.stride_adj, ND,
           (int)lean_sort, (int)level1_quads, n_out);
}
