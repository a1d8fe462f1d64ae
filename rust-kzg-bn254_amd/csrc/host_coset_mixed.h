// host_coset_mixed.h — the host side of coset-proof batches of MIXED blob shapes (capi_coset.hip kzg_verify_multiproof_batch_mixed,
// kzg_coset_interpolate_rlc_mixed; multiverify.hip runs the plan): the argument checks in their documented order, the permutation of
// the items by class and their value offsets, the groups of equal chunk length, and the planner that divides the workgroups of
// k_coset_interp_mixed among the classes and lays out the rows of k_coset_sum_rows_mixed.  A class is a pair (n, l): cosets of l points
// of the n-point domain.  Pure host code (no HIP, no engine.h): also compiled alone by g++ (tests/hostcheck/cosetmixedcheck.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/kzg_bn254_mi355x.h"

namespace kzg_host {

constexpr size_t MIXED_MAX_CLASSES = 512;
constexpr uint32_t MIXED_MAX_GROUPS = 1024;            // workgroups of the two interpolation launches together (coset_kernels.h MV_MAX_GROUPS)
constexpr size_t MIXED_LDS_MAX_L = 1024;               // longer cosets: one ntt_run per coset (coset_kernels.h MV_LDS_MAX_L)
constexpr size_t MIXED_MAX_VALUES = (size_t)1 << 28;   // sum of the items' chunk lengths
constexpr uint32_t MIXED_NO_ITEM = 0xFFFFFFFFu;        // (a value offset is below 2^28)

// the domain / chunk table of kzg_compute_multiproofs, in the documented order
inline int32_t coset_domain_check(size_t n, size_t chunk_len) {
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 24)) return KZG_ERR_DOMAIN;
    if (n == 1 || chunk_len == 0 || (chunk_len & (chunk_len - 1)) != 0 || chunk_len > n / 2) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}

// What a workgroup of k_coset_interp_mixed reads about its class (device table, one entry per class)
struct MixedClassDev {
    uint32_t first, count;        // its items: perm[first .. first + count)
    uint32_t tiles;               // ceil(count / (E / l))
    uint32_t wg_first, wg_count;  // its workgroups within its launch: blockIdx.x in [wg_first, wg_first + wg_count); tile stride wg_count
    uint32_t row_off;             // int32 words: its wg_count partial rows of 9 planes of l words each follow one another from here
    uint32_t log_l, log_n;
};
// A row of k_coset_sum_rows_mixed: it contributes to the columns t < 2^log_l.  Plane rows (9 planes of l limb words, what a workgroup
// of k_coset_interp_mixed leaves) are addressed in int32 words, wire rows (l canonical wire elements, the per-coset route) in elements.
struct MixedRow { uint32_t off; uint32_t log_l_kind; };   // log_l | (wire row ? 0x100 : 0)

struct MixedLongItem { uint32_t item, val_off, row_off, log_l, log_n; };   // item: the caller's index
struct MixedLenGroup { size_t l, first, count; size_t g2_class; };   // items perm[first .. first + count) have chunk length l; g2_class: the first class of that length

struct MixedPlan {
    size_t n_classes = 0, count = 0, l_max = 0, total_values = 0;
    int log_n_max = 0;                         // over the non-empty classes
    std::vector<uint32_t> order;               // the classes by (chunk length, class index)
    std::vector<uint32_t> perm;                // the items by (chunk length, class index, caller's position): sorted by class AND by chunk length
    std::vector<uint32_t> val_off;             // per item, caller's index: where its values start in the ragged array
    std::vector<MixedClassDev> cls;            // per class, caller's numbering (empty classes: count = 0, no workgroup)
    std::vector<uint32_t> wg_class[2];         // launch 0 (l <= 512, tiles of 512 values) and 1 (l = 1024, tiles of 1024): the class of each workgroup
    size_t lds_bytes[2] = {0, 0};              // dynamic LDS of each launch: the largest of its classes
    std::vector<MixedLongItem> long_items;     // the items with l > 1024, in perm order; the wire row of entry j starts at wire element long_items[j].row_off
    std::vector<MixedRow> rows;                // plane rows first, then wire rows
    size_t plane_words = 0, wire_elems = 0;
    std::vector<MixedLenGroup> lens;           // the distinct chunk lengths that have items, ascending
};

// dynamic LDS of k_coset_interp_mixed<E / 256> for a class of chunk length l: x 9 x E | scale 9 x (E / l) | stage twiddles 9 x max(l / 2, 1) |
// coset index E / l | value offset E / l   (9 = NL, the limb planes of field29.h; at most 55 KiB: E = 1024, l = 1024 is 55 340 bytes)
inline size_t mixed_interp_lds_bytes(uint32_t E, size_t l) {
    const size_t cpt = E / l;
    return ((size_t)9 * E + (size_t)9 * cpt + (size_t)9 * (l / 2 > 1 ? l / 2 : 1) + 2 * cpt) * 4;
}

// The checks of the mixed entries that need no device, in the documented order (kzg_verify_multiproof_batch_mixed: steps 1 to 8).  handles_bad: a
// null pointer, or an SRS of another context or a Lagrange handle (decided by the caller, who knows the handles).  srs_len: points of the SRS
// (SIZE_MAX: no SRS in this entry).  commitment_indices / g2_tau_l may be null (kzg_coset_interpolate_rlc_mixed has neither).
inline int32_t mixed_checks(bool handles_bad, const uint64_t* class_n, const uint64_t* class_chunk_len, size_t n_classes, size_t srs_len, size_t n_commitments,
                            const uint64_t* commitment_indices, const uint64_t* class_indices, const uint64_t* coset_indices, size_t count,
                            const uint64_t* g2_tau_l, size_t* out_l_max, size_t* out_total) {
    if (handles_bad) return KZG_ERR_INVALID_ARG;
    if (n_classes == 0 && count > 0) return KZG_ERR_INVALID_ARG;
    if (n_classes > MIXED_MAX_CLASSES) return KZG_ERR_TOO_LARGE;
    size_t l_max = 0;
    for (size_t s = 0; s < n_classes; ++s) {
        const int32_t rc = coset_domain_check((size_t)class_n[s], (size_t)class_chunk_len[s]);
        if (rc != KZG_OK) return rc;
        l_max = std::max(l_max, (size_t)class_chunk_len[s]);
    }
    if (l_max > srs_len) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    for (size_t i = 0; i < count; ++i) {
        const uint64_t s = class_indices[i];
        if (s >= n_classes || coset_indices[i] >= class_n[s] / class_chunk_len[s]) return KZG_ERR_INVALID_ARG;
        if (commitment_indices && commitment_indices[i] >= n_commitments) return KZG_ERR_INVALID_ARG;
    }
    size_t total = 0;
    for (size_t i = 0; i < count; ++i) {
        total += (size_t)class_chunk_len[class_indices[i]];            // (each term <= 2^23: no overflow before the test)
        if (total > MIXED_MAX_VALUES) return KZG_ERR_TOO_LARGE;
    }
    if (g2_tau_l)
        for (size_t s = 1; s < n_classes; ++s)
            for (size_t q = 0; q < s; ++q)
                if (class_chunk_len[q] == class_chunk_len[s]) {
                    if (memcmp(g2_tau_l + 16 * q, g2_tau_l + 16 * s, 128) != 0) return KZG_ERR_INVALID_ARG;
                    break;                                             // (q agrees with every earlier class of this length)
                }
    *out_l_max = l_max;
    *out_total = total;
    return KZG_OK;
}

// The value offsets alone (the transcript needs nothing else): off[i] = sum_{j < i} l_{s_j}; returns the total
inline size_t mixed_value_offsets(const uint64_t* class_chunk_len, const uint64_t* class_indices, size_t count, std::vector<uint32_t>* off) {
    off->resize(count);
    size_t total = 0;
    for (size_t i = 0; i < count; ++i) { (*off)[i] = (uint32_t)total; total += (size_t)class_chunk_len[class_indices[i]]; }
    return total;
}

// The planner.  The arguments have passed mixed_checks.  At most MIXED_MAX_GROUPS workgroups go to the non-empty classes of l <= 1024 in
// proportion to their work, tiles x max(log l, 1) (a tile costs its log l stages; l = 1 has none and counts as one): every such class gets
// one workgroup, the rest of the budget is split by floor(share), and no class gets more workgroups than it has tiles.  When every tile can
// have a workgroup of its own it gets one.
inline void mixed_plan(const uint64_t* class_n, const uint64_t* class_chunk_len, size_t n_classes, const uint64_t* class_indices, size_t count, MixedPlan* p) {
    p->n_classes = n_classes; p->count = count; p->l_max = 0; p->log_n_max = 0;
    for (size_t s = 0; s < n_classes; ++s) p->l_max = std::max(p->l_max, (size_t)class_chunk_len[s]);
    p->total_values = mixed_value_offsets(class_chunk_len, class_indices, count, &p->val_off);
    p->order.resize(n_classes);
    for (size_t s = 0; s < n_classes; ++s) p->order[s] = (uint32_t)s;
    std::stable_sort(p->order.begin(), p->order.end(), [&](uint32_t a, uint32_t b) { return class_chunk_len[a] < class_chunk_len[b]; });
    // counting sort of the items by class, the classes in `order`
    p->cls.assign(n_classes, MixedClassDev{0, 0, 0, 0, 0, 0, 0, 0});
    for (size_t i = 0; i < count; ++i) ++p->cls[class_indices[i]].count;
    uint32_t at = 0;
    for (uint32_t s : p->order) {
        MixedClassDev& c = p->cls[s];
        c.first = at; at += c.count;
        c.log_l = (uint32_t)__builtin_ctzll(class_chunk_len[s]);
        c.log_n = (uint32_t)__builtin_ctzll(class_n[s]);
        if (c.count) p->log_n_max = std::max(p->log_n_max, (int)c.log_n);
    }
    p->perm.resize(count);
    {
        std::vector<uint32_t> next(n_classes);
        for (size_t s = 0; s < n_classes; ++s) next[s] = p->cls[s].first;
        for (size_t i = 0; i < count; ++i) p->perm[next[class_indices[i]]++] = (uint32_t)i;
    }
    // the groups of equal chunk length
    p->lens.clear();
    for (uint32_t s : p->order) {
        const MixedClassDev& c = p->cls[s];
        if (!c.count) continue;
        const size_t l = (size_t)1 << c.log_l;
        if (p->lens.empty() || p->lens.back().l != l) {
            size_t g2_class = s;
            for (size_t q = 0; q < n_classes; ++q) if (class_chunk_len[q] == l) { g2_class = q; break; }
            p->lens.push_back(MixedLenGroup{l, c.first, 0, g2_class});
        }
        p->lens.back().count += c.count;
    }
    // tiles and the division of the workgroups
    uint64_t weight_sum = 0, tile_sum = 0;
    uint32_t tiled = 0;
    for (size_t s = 0; s < n_classes; ++s) {
        MixedClassDev& c = p->cls[s];
        if (!c.count || ((size_t)1 << c.log_l) > MIXED_LDS_MAX_L) continue;
        const uint32_t E = c.log_l == 10 ? 1024u : 512u, cpt = E >> c.log_l;
        c.tiles = (c.count + cpt - 1) / cpt;
        weight_sum += (uint64_t)c.tiles * std::max<uint32_t>(c.log_l, 1);
        tile_sum += c.tiles;
        ++tiled;
    }
    const uint64_t spare = MIXED_MAX_GROUPS - tiled;                   // (tiled <= MIXED_MAX_CLASSES < MIXED_MAX_GROUPS)
    p->wg_class[0].clear(); p->wg_class[1].clear();
    p->lds_bytes[0] = p->lds_bytes[1] = 0;
    p->rows.clear();
    p->plane_words = 0;
    for (uint32_t s : p->order) {
        MixedClassDev& c = p->cls[s];
        if (!c.tiles) continue;
        const uint64_t w = (uint64_t)c.tiles * std::max<uint32_t>(c.log_l, 1);
        const uint64_t want = tile_sum <= MIXED_MAX_GROUPS ? c.tiles : 1 + spare * w / weight_sum;
        const int launch = c.log_l == 10 ? 1 : 0;
        const size_t l = (size_t)1 << c.log_l;
        c.wg_count = (uint32_t)std::min<uint64_t>(want, c.tiles);
        c.wg_first = (uint32_t)p->wg_class[launch].size();
        c.row_off = (uint32_t)p->plane_words;
        for (uint32_t g = 0; g < c.wg_count; ++g) {
            p->wg_class[launch].push_back(s);
            p->rows.push_back(MixedRow{(uint32_t)p->plane_words, c.log_l});
            p->plane_words += 9 * l;
        }
        p->lds_bytes[launch] = std::max(p->lds_bytes[launch], mixed_interp_lds_bytes(launch ? 1024u : 512u, l));
    }
    // the per-coset route: one wire row per item
    p->long_items.clear();
    p->wire_elems = 0;
    for (uint32_t s : p->order) {
        const MixedClassDev& c = p->cls[s];
        if (!c.count || ((size_t)1 << c.log_l) <= MIXED_LDS_MAX_L) continue;
        for (uint32_t j = 0; j < c.count; ++j) {
            const uint32_t i = p->perm[c.first + j];
            p->long_items.push_back(MixedLongItem{i, p->val_off[i], (uint32_t)p->wire_elems, c.log_l, c.log_n});
            p->rows.push_back(MixedRow{(uint32_t)p->wire_elems, c.log_l | 0x100u});
            p->wire_elems += (size_t)1 << c.log_l;
        }
    }
}

}  // namespace kzg_host
