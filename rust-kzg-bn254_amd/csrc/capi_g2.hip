// capi_g2.hip — the G2 part of the C-ABI (include/kzg_bn254_mi355x.h, "G2 on the device"): the device-resident G2 SRS handle, the G2
// MSM over caller bases or a handle, G2 commitments, the blob header (commitment, length commitment, length proof) in one call, the
// headers of many blobs and the batched MSM over shared bases (with the pure query of their plan), the header's verification by two
// pairing checks, the batched verification of headers (subgroup test and weighted sums on the device, one product of pairings), the group sums of such a
// batch and the search for its bad headers (one shared prefix of checks, uploads and weights for the three; host_header_locate.h), the same two verdicts from
// SERIALIZED headers (a second prefix that decodes on the device, headerbytes.hip; the tails are shared) with the headers' encoder and decoder, and the decoders of gnark-compressed G2 points: on the host, and on the device into wire points or a resident
// handle.  The kernels and their drivers are g2msm.hip, g2batch.hip and g2decode.hip; every argument check here runs before any launch.
#include "engine.h"
#include <new>
#include "field29.h"
#include "g2msm_plan.h"
#include "host_curve.h"
#include "host_g2_decode.h"
#include "host_fiat_shamir.h"
#include "host_header_bytes.h"
#include "host_header_locate.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>
#include <cstring>

using namespace kzg;

namespace {

bool is_pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }

// the synchronous calls share slot 0's workspace and stream
bool slot0_busy(kzg_ctx* ctx) {
    if (!ctx->slot_pending[0]) return false;
    ctx->last_error = "a kzg_*_begin on slot 0 is still in flight: call kzg_msm_g1_srs_end(ctx, 0, ..) first";
    return true;
}
void write_g2_identity(uint64_t out[16], uint8_t* out_inf) {
    memset(out, 0, 128);
    if (out_inf) *out_inf = 1;
}
int32_t stage_scalars_g2(kzg_ctx* ctx, const uint64_t* scalars, size_t n, const void** d_out) {
    KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve(n * 32 + 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    *d_out = ctx->msm.scalars.p;
    return KZG_OK;
}
kzg_g2srs* new_handle(kzg_ctx* ctx, size_t n, int32_t* rc) {
    *rc = KZG_OK;
    kzg_g2srs* s = new (std::nothrow) kzg_g2srs();
    if (!s) { *rc = KZG_ERR_INVALID_ARG; return nullptr; }
    s->ctx = ctx;
    s->n = n;
    if (n) {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), n * 128);
        if (e != hipSuccess) { delete s; *rc = set_error(ctx, e, "hipMalloc(g2 srs)"); return nullptr; }
    }
    return s;
}
void drop_handle(kzg_g2srs* s) {
    if (s->d_points) (void)hipFree(s->d_points);
    delete s;
}

// (the caller holds ctx->mu)
int32_t msm_g2_srs_locked(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                          uint64_t out[16], uint8_t* out_inf) {
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n == 0) { write_g2_identity(out, out_inf); return KZG_OK; }
    const void* d_scalars = scalars;
    if (!on_device) { const int32_t rc = stage_scalars_g2(ctx, static_cast<const uint64_t*>(scalars), n, &d_scalars); if (rc != KZG_OK) return rc; }
    const uint4* pts[1] = {srs->d_points + 8 * offset};
    return g2_msm_run(ctx, pts, 1, d_scalars, n, out, out_inf);
}
int32_t msm_g2_srs_common(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                          uint64_t out[16], uint8_t* out_inf) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out || (n && !scalars)) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_POLY_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_g2_srs_locked(ctx, srs, offset, scalars, on_device, n, out, out_inf);
}


// the size of a batch: row 2 of the batched calls' error tables
int32_t g2_batch_size_check(size_t n, size_t count) {
    if (count > ((size_t)1 << 20)) return KZG_ERR_TOO_LARGE;
    if (n && count && n > SIZE_MAX / 32 / count) return KZG_ERR_INVALID_ARG;           // count n 32 bytes of scalars
    return KZG_OK;
}
int32_t msm_g2_srs_batch_common(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* scalars, bool on_device, size_t n, size_t count,
                                uint64_t* out, uint8_t* out_inf) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out || (n && count && !scalars)) return KZG_ERR_INVALID_ARG;
    { const int32_t rc = g2_batch_size_check(n, count); if (rc != KZG_OK) return rc; }
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_POLY_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (count == 0) return KZG_OK;
    if (n == 0) {
        memset(out, 0, count * 128);
        if (out_inf) memset(out_inf, 1, count);
        return KZG_OK;
    }
    const void* d_scalars = scalars;
    if (!on_device) { const int32_t rc = stage_scalars_g2(ctx, static_cast<const uint64_t*>(scalars), count * n, &d_scalars); if (rc != KZG_OK) return rc; }
    const uint4* pts[1] = {srs->d_points + 8 * offset};
    uint64_t* outs[1] = {out};
    uint8_t* infs[1] = {out_inf};
    return g2_msm_batch_run(ctx, pts, 1, d_scalars, n, count, outs, infs);
}

// ---- batches of blob headers: what kzg_verify_length_proof_batch, kzg_header_group_sums and kzg_verify_length_proof_batch_locate share --------
// Where a batch of headers stands once the shared prefix has run: every input checked (rows 1-7 of the header's table), the G2 points on the
// device, the weights at hand.
struct HeaderStage {
    std::unique_lock<std::mutex> lk;             // ctx->mu: taken behind row 5, held until the entry is done with the device
    std::vector<uint8_t> length_class;           // [header] -> the position of its claimed length in shift_lens
    std::vector<kzg_host::G1> shifts;            // T_s, on the curve
    const uint4* d_points = nullptr;             // ctx->msm.bases, device format: C2_0, pi2_0, C2_1, pi2_1, ..
    size_t n_points = 0;
    const uint64_t* weights = nullptr;           // wire form: r_0 .. r_(count-1), rho; supplied or derived (then in `derived`)
    std::vector<uint64_t> derived, canon;        // canon: the same count + 1 values as canonical words
    int bits = 0;                                // the bit length of the largest r_i: the trip count of the G2 chains
    Clock::time_point t0, t1, t2;                // start of row 5, the end of the on-twist test, the end of the subgroup test
    // the prefix for serialized headers: the commitments are on the device too (ctx->ml[5], device format), decoded where the G1 sums read
    // them, and no tail uploads them; t1 = the end of the decode, t2 = the end of the item digests
    const uint4* d_commitments = nullptr;
    bool from_bytes = false;
    // the weights as the tails read them: wire form for the G1 side, canonical words for the G2 chains, the chains' trip count
    void set_weights(const uint64_t* weights_mont, size_t count) {
        weights = weights_mont;
        canon.resize((count + 1) * 4);
        bits = 0;
        for (size_t i = 0; i <= count; ++i) {
            uint64_t* k = canon.data() + 4 * i;
            kzg_host::fr_wire_to_canonical(weights_mont + 4 * i, k);
            if (i == count) break;                                  // rho multiplies on the host
            for (int w = 3; w >= 0; --w) if (k[w]) { bits = std::max(bits, 64 * w + 64 - __builtin_clzll(k[w])); break; }
        }
    }
};

// Rows 1-4 (host_header_locate.h: with the group rows of a grouped entry), *empty = (count == 0) and nothing else done; else rows 5-7 and the
// weights.  `who` names the entry in the lines for kzg_ctx_last_error.
int32_t header_batch_prefix(const char* who, kzg_ctx* ctx, bool output_null, const uint64_t* commitments_xy, const uint64_t* length_commitments,
                            const uint64_t* length_proofs, const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens,
                            const uint64_t* g1_tau_shifts_xy, size_t n_shifts, const uint64_t* weights_mont, const HeaderGrouping& grp, uint64_t* bad_index,
                            bool* empty, HeaderStage* st) {
    using namespace kzg_host;
    // 1-4 (and 4a, 4b)
    int32_t rc = header_batch_checks(!ctx || output_null, commitments_xy, length_commitments, length_proofs, claimed_lens, count, shift_lens, g1_tau_shifts_xy, n_shifts,
                                     grp, &st->length_class, bad_index);
    if (rc != KZG_OK) return rc;
    *empty = count == 0;
    if (count == 0) return KZG_OK;
    st->t0 = Clock::now();
    // 5. G1 inputs on the curve: the commitments (the header's index), then the shifts (the shift's position in the list)
    {
        std::atomic<uint64_t> first_bad{UINT64_MAX};
        const size_t per = 256, jobs = (count + per - 1) / per;
        auto body = [&](size_t j) {
            for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
                if (g1_on_curve(g1_from_wire(commitments_xy + 8 * i))) continue;
                uint64_t cur = first_bad.load();
                while (i < cur && !first_bad.compare_exchange_weak(cur, (uint64_t)i)) {}
                return;
            }
        };
        if (jobs > 1) host_parallel_for(jobs, body); else body(0);
        if (first_bad.load() != UINT64_MAX) { if (bad_index) *bad_index = first_bad.load(); return KZG_ERR_G1_NOT_ON_CURVE; }
    }
    st->shifts.resize(n_shifts);
    for (size_t g = 0; g < n_shifts; ++g) {
        st->shifts[g] = g1_from_wire(g1_tau_shifts_xy + 8 * g);
        if (!g1_on_curve(st->shifts[g])) { if (bad_index) *bad_index = (uint64_t)g; return KZG_ERR_G1_NOT_ON_CURVE; }
    }
    st->lk = std::unique_lock<std::mutex>(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    // 6. G2 inputs on the twist: uploaded as C2_0, pi2_0, C2_1, pi2_1, ..: point j belongs to header j / 2, C2 in front of pi2
    const size_t n_points = 2 * count;
    std::vector<uint64_t> inter(n_points * 16);
    for (size_t i = 0; i < count; ++i) { memcpy(inter.data() + 32 * i, length_commitments + 16 * i, 128); memcpy(inter.data() + 32 * i + 16, length_proofs + 16 * i, 128); }
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_points * 128));
    st->d_points = ctx->msm.bases.as<uint4>();
    st->n_points = n_points;
    int64_t bad = -1;
    rc = g2_upload_points(ctx, inter.data(), n_points, ctx->msm.bases.as<uint4>(), &bad);
    if (rc != KZG_OK) return rc;
    if (bad >= 0) {
        if (bad_index) *bad_index = (uint64_t)bad / 2;
        ctx->last_error = std::string(who) + ": the length " + (bad & 1 ? "proof" : "commitment") + " of header " + std::to_string(bad / 2) + " is not on the twist";
        return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    }
    st->t1 = Clock::now();
    // 7. G2 inputs in the order-r subgroup
    rc = g2_subgroup_check(ctx, st->d_points, n_points, &bad);
    if (rc != KZG_OK) return rc;
    if (bad >= 0) {
        if (bad_index) *bad_index = (uint64_t)bad / 2;
        ctx->last_error = std::string(who) + ": the length " + (bad & 1 ? "proof" : "commitment") + " of header " + std::to_string(bad / 2) + " is not in the order-r subgroup";
        return KZG_ERR_NOT_ON_CURVE;
    }
    st->t2 = Clock::now();
    // the weights r_0 .. r_(count-1), rho: wire form for the G1 side, canonical words for the G2 chains
    if (!weights_mont) {
        st->derived.resize((count + 1) * 4);
        header_batch_weights_host(commitments_xy, length_commitments, length_proofs, claimed_lens, count, shift_lens, g1_tau_shifts_xy, n_shifts, st->derived.data(), host_parallel_for);
        weights_mont = st->derived.data();
    }
    st->set_weights(weights_mont, count);
    return KZG_OK;
}

// The same stage from SERIALIZED headers (kzg_verify_length_proof_batch_bytes, kzg_verify_length_proof_batch_locate_bytes): rows 1-4 on the
// host, slot 0, the shifts on the curve (*bad_array = 3), then one decode pass on the device (headerbytes.hip): the G2 elements land
// subgroup-checked where the chains read them (ONE 63-bit chain per element: the decoder's is the only one), the commitments where the G1
// sums read them, nothing decoded returns to the host.  A refused element sets *bad_array (0 commitment, 1 length commitment, 2 length
// proof) and *bad_index.  Derived weights hash the items on the device (32 B per header come down for the batch hash, which stays here).
int32_t header_batch_prefix_bytes(const char* who, kzg_ctx* ctx, bool output_null, const uint8_t* commitments_be, const uint8_t* length_commitments_be,
                                  const uint8_t* length_proofs_be, const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens,
                                  const uint64_t* g1_tau_shifts_xy, size_t n_shifts, const uint64_t* weights_mont, const HeaderGrouping& grp, uint64_t* bad_index,
                                  int32_t* bad_array, bool* empty, HeaderStage* st) {
    using namespace kzg_host;
    int32_t rc = header_batch_checks(!ctx || output_null, commitments_be, length_commitments_be, length_proofs_be, claimed_lens, count, shift_lens, g1_tau_shifts_xy,
                                     n_shifts, grp, &st->length_class, bad_index);
    if (rc != KZG_OK) return rc;
    *empty = count == 0;
    if (count == 0) return KZG_OK;
    st->t0 = Clock::now();
    st->from_bytes = true;
    st->lk = std::unique_lock<std::mutex>(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    st->shifts.resize(n_shifts);
    for (size_t g = 0; g < n_shifts; ++g) {
        st->shifts[g] = g1_from_wire(g1_tau_shifts_xy + 8 * g);
        if (!g1_on_curve(st->shifts[g])) { if (bad_index) *bad_index = (uint64_t)g; if (bad_array) *bad_array = 3; return KZG_ERR_G1_NOT_ON_CURVE; }
    }
    const size_t n_points = 2 * count;
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_points * 128));
    KZG_HIP_TRY(ctx, ctx->ml[5].reserve(count * 64));
    HeaderBytesDecode job;
    job.commitments_be = commitments_be; job.length_commitments_be = length_commitments_be; job.length_proofs_be = length_proofs_be;
    job.count = count;
    job.d_commitments = ctx->ml[5].as<uint4>();
    job.d_g2 = ctx->msm.bases.as<uint4>();
    rc = header_bytes_decode(ctx, &job);
    if (rc != KZG_OK) return rc;
    rc = header_bytes_status(ctx, who, job, bad_index, bad_array);
    if (rc != KZG_OK) return rc;
    st->d_points = job.d_g2;
    st->n_points = n_points;
    st->d_commitments = job.d_commitments;
    st->t1 = Clock::now();
    if (!weights_mont) {
        std::vector<uint8_t> data = header_batch_transcript(count, shift_lens, g1_tau_shifts_xy, n_shifts);
        rc = header_item_digests_run(ctx, job.d_commitments_be, job.d_g2, claimed_lens, count, data.data() + header_batch_head(n_shifts));
        if (rc != KZG_OK) return rc;
        st->derived.resize((count + 1) * 4);
        header_weights_from_transcript(data, count, st->derived.data(), host_parallel_for);
        weights_mont = st->derived.data();
    }
    st->t2 = Clock::now();
    st->set_weights(weights_mont, count);
    return KZG_OK;
}

// The device's part of the grouped entries: per non-empty group U_g (XYZZ), per non-empty (group, length class) W_{g,s} and per non-empty
// group Pi_g (affine wire points), in the segment order of the two plans.
struct HeaderGroupSums {
    LocatePlan g1_plan, g2_plan;                 // the headers by group; the 2 count G2 points by the composite key of host_header_locate.h
    std::vector<kzg_host::Xyzz> u;               // per segment of g1_plan
    std::vector<uint64_t> q;                     // per segment of g2_plan: 16 u64
    double ms_g2 = 0, ms_g1 = 0;
};

// The stage has passed header_batch_prefix with the grouping; count > 0.  The G2 points are on the device already; the commitments go up
// here, validated again on their way into the device format (they have passed row 5), unless the stage holds them (serialized headers: they
// were decoded into ctx->ml[5], and commitments_xy is null).
int32_t header_group_sums_core(kzg_ctx* ctx, const HeaderStage& st, const uint64_t* commitments_xy, size_t count, size_t n_shifts, const uint64_t* group_indices,
                               size_t n_groups, HeaderGroupSums* out) {
    const auto t0 = Clock::now();
    std::vector<uint64_t> keys;
    header_locate_keys(group_indices, st.length_class.data(), count, n_groups, n_shifts, &keys);
    int32_t rc = locate_plan(keys.data(), keys.size(), header_n_keys(n_groups, n_shifts), &out->g2_plan);
    if (rc != KZG_OK) return rc;
    out->q.resize(16 * out->g2_plan.segs.size());
    rc = g2_locate_segment_sums(ctx, st.d_points, st.n_points, out->g2_plan, reinterpret_cast<const uint32_t*>(st.canon.data()), count, st.bits, out->q.data());
    if (rc != KZG_OK) return rc;
    const auto t1 = Clock::now();
    rc = locate_plan(group_indices, count, n_groups, &out->g1_plan);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, ctx->ml[4].reserve(count * 32));
    if (!st.d_commitments) {
        KZG_HIP_TRY(ctx, ctx->ml[5].reserve(count * 64));
        uint32_t off_curve = 0;
        rc = upload_points(ctx, commitments_xy, count, ctx->ml[5].as<uint4>(), ctx->msm.bases_wire, &off_curve);
        if (rc != KZG_OK) return rc;
        if (off_curve) return KZG_ERR_G1_NOT_ON_CURVE;
    }
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->ml[4].p, st.weights, count * 32, hipMemcpyHostToDevice, ctx->stream));
    rc = locate_upload_plan(ctx, out->g1_plan);
    if (rc != KZG_OK) return rc;
    out->u.resize(out->g1_plan.segs.size());
    static_assert(sizeof(kzg_host::Xyzz) == 128, "the device leaves 16 wire words per sum");
    rc = locate_group_sums_g1_device(ctx, ctx->ml[5].as<uint4>(), ctx->ml[4].as<uint4>(), out->g1_plan, reinterpret_cast<uint64_t*>(out->u.data()));
    if (rc != KZG_OK) return rc;
    out->ms_g2 = ms_between(t0, t1);
    out->ms_g1 = ms_between(t1, Clock::now());
    return KZG_OK;
}

// The tail of the batch entries: the stage has passed a prefix, count > 0.  commitments_xy: the wire commitments, or null when the stage holds
// them on the device.  Synchronised on return.
int32_t header_verify_tail(kzg_ctx* ctx, const HeaderStage& st, const uint64_t* commitments_xy, size_t count, size_t n_shifts, int32_t* out_ok) {
    using namespace kzg_host;
    auto ms = ms_between;
    const uint64_t* weights_mont = st.weights;
    int32_t rc;
    const std::vector<uint8_t>& group = st.length_class;
    const std::vector<G1>& shifts = st.shifts;
    const std::vector<uint64_t>& canon = st.canon;
    const uint4* d_points = st.d_points;
    const size_t n_points = st.n_points;
    const int bits = st.bits;
    const auto t0 = st.t0, t1 = st.t1, t2 = st.t2;
    // lanes: the C2 of every group in the list's order, each group padded to whole tiles of 64, then every pi2
    std::vector<size_t> group_count(n_shifts, 0), tile_begin(n_shifts + 2, 0);
    for (size_t i = 0; i < count; ++i) ++group_count[group[i]];
    for (size_t g = 0; g < n_shifts; ++g) tile_begin[g + 1] = tile_begin[g] + (group_count[g] + 63) / 64;
    tile_begin[n_shifts + 1] = tile_begin[n_shifts] + (count + 63) / 64;
    const size_t tiles = tile_begin[n_shifts + 1];
    std::vector<uint32_t> lanes(tiles * 64, 0xFFFFFFFFu);
    {
        std::vector<size_t> next(n_shifts);
        for (size_t g = 0; g < n_shifts; ++g) next[g] = tile_begin[g] * 64;
        for (size_t i = 0; i < count; ++i) { lanes[next[group[i]]++] = (uint32_t)(2 * i); lanes[tile_begin[n_shifts] * 64 + i] = (uint32_t)(2 * i + 1); }
    }
    std::vector<uint64_t> tile_sums(tiles * 16);
    rc = g2_weighted_tile_sums(ctx, d_points, n_points, lanes.data(), lanes.size(), reinterpret_cast<const uint32_t*>(canon.data()), count, 1, bits, tile_sums.data());
    if (rc != KZG_OK) return rc;
    const auto t3 = Clock::now();
    // U = sum r_i C_i: the variable-base G1 MSM of the batched verifiers
    uint64_t u_xy[8];
    uint8_t u_inf = 0;
    if (st.d_commitments) {
        const void* d_scalars;
        rc = stage_scalars_g2(ctx, weights_mont, count, &d_scalars);
        if (rc == KZG_OK) rc = msm_run_batch(ctx, st.d_commitments, d_scalars, count, 1, u_xy, &u_inf);
    } else {
        rc = msm_g1_batch_locked(ctx, commitments_xy, weights_mont, count, 1, u_xy, &u_inf, nullptr);
    }
    if (rc != KZG_OK) return rc;
    const auto t4 = Clock::now();
    // W_g, Pi: the tiles of one sum added in Jacobian coordinates, one inversion per sum
    auto sum_tiles = [&](size_t lo, size_t hi) {
        G2Jac acc; acc.inf = true; acc.X = {fq_zero(), fq_zero()}; acc.Y = acc.X; acc.Z = acc.X;
        for (size_t t = lo; t < hi; ++t) acc = g2j_madd(acc, g2_from_wire(tile_sums.data() + 16 * t));
        if (acc.inf) return g2_inf();
        const Fq2 zi = inv(acc.Z), zi2 = sqr(zi);
        G2 r; r.inf = false;
        r.x = mul(acc.X, zi2);
        r.y = mul(acc.Y, mul(zi2, zi));
        return r;
    };
    std::vector<G2> W(n_shifts);
    G2 S = g2_inf();
    for (size_t g = 0; g < n_shifts; ++g) { W[g] = sum_tiles(tile_begin[g], tile_begin[g + 1]); S = g2_add(S, W[g]); }
    const G2 Pi = sum_tiles(tile_begin[n_shifts], tile_begin[n_shifts + 1]);
    // e(U, G2) e(-G1, S + [rho]Pi) prod_g e([rho]T_g, W_g) == 1
    const uint64_t* rho = canon.data() + 4 * count;
    std::vector<G1> ps;
    std::vector<G2> qs;
    G1 g1; g1.x = FQ_ONE; g1.y = FQ_TWO; g1.inf = false;
    G1 U = g1_from_wire(u_xy);
    if (u_inf) U.inf = true;
    ps.push_back(U); qs.push_back(g2_generator());
    ps.push_back(g1_neg(g1)); qs.push_back(g2_add(S, g2_mul(Pi, rho)));
    for (size_t g = 0; g < n_shifts; ++g) {
        if (group_count[g] == 0) continue;
        ps.push_back(g1_mul(shifts[g], rho)); qs.push_back(W[g]);
    }
    *out_ok = pairings_product_is_one(ps.data(), qs.data(), (int)ps.size(), host_parallel_for) ? 1 : 0;
    if (opts().vb_trace && st.from_bytes) {
        fprintf(stderr, "  verify_length_proof_batch_bytes count=%zu groups=%zu bits=%d: checks + decode (staging, uploads, decode kernels with the subgroup chain) %.3f ms, "
                "digests + weights %.3f ms, weighted sums %.3f ms, G1 MSM %.3f ms, host sums + pairing %.3f ms\n",
                count, n_shifts, bits, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, Clock::now()));
    } else if (opts().vb_trace) {
        fprintf(stderr, "  verify_length_proof_batch count=%zu groups=%zu bits=%d: checks + upload + on-twist %.3f ms, subgroup %.3f ms, weights + weighted sums %.3f ms, G1 MSM %.3f ms, host sums + pairing %.3f ms\n",
                count, n_shifts, bits, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, Clock::now()));
    }
    return KZG_OK;
}


// The tail of the locate entries: the stage has passed a prefix with the grouping, count > 0; commitments_xy as for header_verify_tail.
int32_t header_locate_tail(kzg_ctx* ctx, HeaderStage& st, const uint64_t* commitments_xy, size_t count, size_t n_shifts, const uint64_t* group_indices, size_t n_groups,
                           uint8_t* out_group_ok, size_t* out_bad_groups, size_t* out_pairing_checks) {
    using namespace kzg_host;
    int32_t rc;
    const auto t_sums = Clock::now();
    HeaderGroupSums gs;
    rc = header_group_sums_core(ctx, st, commitments_xy, count, n_shifts, group_indices, n_groups, &gs);
    if (rc != KZG_OK) return rc;
    st.lk.unlock();                                                  // the rest is host work
    const auto t_host = Clock::now();
    // the leaves: U_g on the left, (Pi_g, W_{g,s} for the classes present) on the right
    const HeaderClasses cls = header_present_classes(st.length_class.data(), count, n_shifts);
    using Sums = HeaderSums<Xyzz, G2Jac>;
    std::vector<Sums> lhs, rhs;
    header_assemble(gs.g1_plan, gs.g2_plan, n_groups, n_shifts, cls, [&](size_t j) { return gs.u[j]; },
                    [&](size_t j) { return g2j_from_affine(g2_from_wire(gs.q.data() + 16 * j)); }, xyzz_inf(), g2j_inf(), &lhs, &rhs);
    // what every test multiplies: rho on the G1 side, once per call
    const uint64_t* rho = st.canon.data() + 4 * count;
    G1 g1; g1.x = FQ_ONE; g1.y = FQ_TWO; g1.inf = false;
    HeaderFixed<G1, G2> fx;
    fx.g2 = g2_generator();
    fx.neg_g1 = g1_neg(g1);
    fx.neg_rho_g1 = g1_neg(g1_mul(g1, rho));
    for (uint32_t s : cls.present) fx.rho_shift.push_back(g1_mul(st.shifts[s], rho));
    struct OpsA {
        Xyzz zero() const { return xyzz_inf(); }
        Xyzz add(const Xyzz& a, const Xyzz& b) const { return xyzz_add(a, b); }
        Xyzz sub(const Xyzz& a, Xyzz b) const { b.y = neg(b.y); return xyzz_add(a, b); }
    };
    struct OpsB {
        G2Jac zero() const { return g2j_inf(); }
        G2Jac add(const G2Jac& a, const G2Jac& b) const { return g2j_add(a, b); }
        G2Jac sub(const G2Jac& a, const G2Jac& b) const { return g2j_add(a, g2j_neg(b)); }
    };
    bool first = true;
    auto t_search = t_host;
    auto holds = [&](const Sums& l, const Sums& r) {
        if (first) { first = false; t_search = Clock::now(); }      // the prefix sums end where the first test begins
        uint64_t a[8];
        uint8_t u_inf = 0;
        xyzz_to_affine(l.u, a, &u_inf);
        G1 U = g1_from_wire(a);
        if (u_inf) U.inf = true;
        std::vector<G2> q(1 + cls.present.size(), g2_inf());
        G2Jac sum_w = g2j_inf();
        for (size_t k = 0; k < r.q.size() && k < q.size(); ++k) {
            q[k] = g2j_to_affine(r.q[k]);
            if (k) sum_w = g2j_add(sum_w, r.q[k]);
        }
        std::vector<G1> ps;
        std::vector<G2> qs;
        header_pairs(fx, U, q, g2j_to_affine(sum_w), &ps, &qs);
        return pairings_product_is_one(ps.data(), qs.data(), (int)ps.size(), host_parallel_for);
    };
    size_t bad = 0;
    const size_t checks = locate_search(lhs.data(), rhs.data(), n_groups, HeaderSumOps<Xyzz, G2Jac, OpsA, OpsB>(), holds, out_group_ok, &bad);
    *out_bad_groups = bad;
    if (out_pairing_checks) *out_pairing_checks = checks;
    if (opts().vb_trace) {
        char parts[96] = "";
        if (st.from_bytes) snprintf(parts, sizeof parts, " (checks + decode %.3f ms, digests + weights %.3f ms)", ms_between(st.t0, st.t1), ms_between(st.t1, st.t2));
        fprintf(stderr, "  verify_length_proof_batch_locate%s count=%zu groups=%zu classes=%zu bits=%d: shared prefix%s %.3f ms, G2 group sums %.3f ms, G1 group sums %.3f ms, "
                "host sums %.3f ms, search %.3f ms, %zu pairing checks, %zu bad groups\n", st.from_bytes ? "_bytes" : "",
                count, n_groups, cls.present.size(), st.bits, parts, ms_between(st.t0, t_sums), gs.ms_g2,
                gs.ms_g1, ms_between(t_host, t_search), ms_between(t_search, Clock::now()), checks, bad);
    }
    return KZG_OK;
}

}  // namespace

extern "C" {

int32_t kzg_g2srs_upload(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n_points, kzg_g2srs** out, uint64_t* bad_index) {
    if (!ctx || !out || (n_points && !g2_mont)) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    int32_t rc;
    kzg_g2srs* s = new_handle(ctx, n_points, &rc);
    if (!s) return rc;
    int64_t bad = -1;
    rc = g2_upload_points(ctx, g2_mont, n_points, s->d_points, &bad);
    if (rc == KZG_OK && bad >= 0) {
        if (bad_index) *bad_index = (uint64_t)bad;
        rc = KZG_ERR_NOT_ON_CURVE;
    }
    if (rc != KZG_OK) { drop_handle(s); return rc; }
    *out = s;
    return KZG_OK;
}

int32_t kzg_g2srs_generate(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n_points, kzg_g2srs** out) {
    if (!ctx || !out || !tau_mont) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    kzg_g2srs* s = new_handle(ctx, n_points, &rc);
    if (!s) return rc;
    rc = g2_generate_points(ctx, tau_mont, first_power, n_points, s->d_points);
    if (rc != KZG_OK) { drop_handle(s); return rc; }
    *out = s;
    return KZG_OK;
}

int32_t kzg_g2srs_download(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, size_t n, uint64_t* out_g2_mont) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || (n && !out_g2_mont)) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    return g2_download_points(ctx, srs->d_points + 8 * offset, n, out_g2_mont);
}

size_t kzg_g2srs_len(const kzg_g2srs* srs) { return srs ? srs->n : 0; }

void kzg_g2srs_free(kzg_g2srs* srs) {
    if (!srs) return;
    if (srs->d_points) { (void)hipSetDevice(srs->ctx->device); (void)hipFree(srs->d_points); }
    delete srs;
}

int32_t kzg_msm_g2(kzg_ctx* ctx, const uint64_t* bases_g2_mont, size_t n_bases, const uint64_t* scalars_mont, size_t n_scalars,
                   uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    if (!ctx || !out_g2_mont) return KZG_ERR_INVALID_ARG;
    if (n_bases != n_scalars) return KZG_ERR_MSM_LENGTH_MISMATCH;
    if (n_bases && (!bases_g2_mont || !scalars_mont)) return KZG_ERR_INVALID_ARG;
    if (n_bases > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n_bases == 0) { write_g2_identity(out_g2_mont, out_is_infinity); return KZG_OK; }
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_bases * 128));
    int64_t bad = -1;
    int32_t rc = g2_upload_points(ctx, bases_g2_mont, n_bases, ctx->msm.bases.as<uint4>(), &bad);
    if (rc != KZG_OK) return rc;
    if (bad >= 0) { ctx->last_error = "kzg_msm_g2: base " + std::to_string(bad) + " is not on the twist"; return KZG_ERR_NOT_ON_CURVE; }
    const void* d_scalars;
    rc = stage_scalars_g2(ctx, scalars_mont, n_scalars, &d_scalars);
    if (rc != KZG_OK) return rc;
    const uint4* pts[1] = {ctx->msm.bases.as<uint4>()};
    return g2_msm_run(ctx, pts, 1, d_scalars, n_bases, out_g2_mont, out_is_infinity);
}

int32_t kzg_msm_g2_srs(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n,
                       uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    return msm_g2_srs_common(ctx, srs, offset, scalars_mont, false, n, out_g2_mont, out_is_infinity);
}
int32_t kzg_msm_g2_srs_device(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* d_scalars_mont, size_t n,
                              uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    return msm_g2_srs_common(ctx, srs, offset, d_scalars_mont, true, n, out_g2_mont, out_is_infinity);
}

int32_t kzg_commit_g2_coeff_form(kzg_ctx* ctx, const kzg_g2srs* srs, const uint64_t* coeffs_mont, size_t n,
                                 uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    return msm_g2_srs_common(ctx, srs, 0, coeffs_mont, false, n, out_g2_mont, out_is_infinity);       // n > len -> KZG_ERR_POLY_LENGTH
}

int32_t kzg_commit_g2_eval_form(kzg_ctx* ctx, const kzg_g2srs* srs, const uint64_t* evals_mont, size_t n,
                                uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out_g2_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (!is_pow2(n)) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->poly[0].a.p, evals_mont, n * 32, hipMemcpyHostToDevice, ctx->stream));
    const int32_t rc = ntt_run(ctx, ctx->poly[0].a.p, n, true);          // coefficients = IFFT(evaluations)
    if (rc != KZG_OK) return rc;
    const uint4* pts[1] = {srs->d_points};
    return g2_msm_run(ctx, pts, 1, ctx->poly[0].a.p, n, out_g2_mont, out_is_infinity);
}

int32_t kzg_commit_with_length_proof(kzg_ctx* ctx, const kzg_srs* g1_srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing,
                                     uint64_t trailing_first_power, uint64_t srs_order, const uint64_t* coeffs_mont, size_t n,
                                     uint64_t claimed_len, uint64_t out_commitment_xy[8], uint64_t out_length_commitment[16],
                                     uint64_t out_length_proof[16]) {
    if (!ctx || !g1_srs || !g2_srs || !g2_trailing || !out_commitment_xy || !out_length_commitment || !out_length_proof || (n && !coeffs_mont))
        return KZG_ERR_INVALID_ARG;
    if (g1_srs->ctx->device != ctx->device || g2_srs->ctx->device != ctx->device || g2_trailing->ctx->device != ctx->device) return KZG_ERR_INVALID_ARG;
    if (!is_pow2(srs_order) || !is_pow2(claimed_len)) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > claimed_len || claimed_len > srs_order) return KZG_ERR_INVALID_ARG;
    // the proof's bases [tau^(N - d + i)]_2, i < n: from this offset of the trailing handle
    if (srs_order - claimed_len < trailing_first_power) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    const uint64_t off = srs_order - claimed_len - trailing_first_power;
    if (off > g2_trailing->n || claimed_len > g2_trailing->n - off) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (n > g1_srs->n || n > g2_srs->n) return KZG_ERR_POLY_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n == 0) {
        memset(out_commitment_xy, 0, 64); memset(out_length_commitment, 0, 128); memset(out_length_proof, 0, 128);
        return KZG_OK;
    }
    const void* d_scalars;
    int32_t rc = stage_scalars_g2(ctx, coeffs_mont, n, &d_scalars);      // the one upload: all three MSMs read it
    if (rc != KZG_OK) return rc;
    rc = msm_srs_locked(ctx, g1_srs, 0, d_scalars, true, n, out_commitment_xy, nullptr, nullptr);
    if (rc != KZG_OK) return rc;
    const uint4* pts[2] = {g2_srs->d_points, g2_trailing->d_points + 8 * off};
    uint64_t out2[32];
    rc = g2_msm_run(ctx, pts, 2, d_scalars, n, out2, nullptr);           // one digit pass and sort, two accumulations
    if (rc != KZG_OK) return rc;
    memcpy(out_length_commitment, out2, 128);
    memcpy(out_length_proof, out2 + 16, 128);
    return KZG_OK;
}

// ---- many blobs in one call: the batched G2 MSM over shared bases (g2msm.hip g2_msm_batch_run) -----------------------------------------
int32_t kzg_msm_g2_srs_batch(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n, size_t count,
                             uint64_t* out_g2_mont, uint8_t* out_is_infinity) {
    return msm_g2_srs_batch_common(ctx, srs, offset, scalars_mont, false, n, count, out_g2_mont, out_is_infinity);
}
int32_t kzg_msm_g2_srs_batch_device(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* d_scalars_mont, size_t n, size_t count,
                                    uint64_t* out_g2_mont, uint8_t* out_is_infinity) {
    return msm_g2_srs_batch_common(ctx, srs, offset, d_scalars_mont, true, n, count, out_g2_mont, out_is_infinity);
}

int32_t kzg_commit_with_length_proof_batch(kzg_ctx* ctx, kzg_srs* g1_srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing,
                                           uint64_t trailing_first_power, uint64_t srs_order, const uint64_t* coeffs_mont, size_t n, size_t count,
                                           uint64_t claimed_len, uint64_t* out_commitments_xy, uint64_t* out_length_commitments,
                                           uint64_t* out_length_proofs) {
    // 1. pointers and devices
    if (!ctx || !g1_srs || !g2_srs || !g2_trailing || !out_commitments_xy || !out_length_commitments || !out_length_proofs || (n && count && !coeffs_mont))
        return KZG_ERR_INVALID_ARG;
    if (g1_srs->ctx->device != ctx->device || g2_srs->ctx->device != ctx->device || g2_trailing->ctx->device != ctx->device) return KZG_ERR_INVALID_ARG;
    // 2. the size of the batch
    { const int32_t rc = g2_batch_size_check(n, count); if (rc != KZG_OK) return rc; }
    // 3. rows 2 to 5 of kzg_commit_with_length_proof
    if (!is_pow2(srs_order) || !is_pow2(claimed_len)) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > claimed_len || claimed_len > srs_order) return KZG_ERR_INVALID_ARG;
    if (srs_order - claimed_len < trailing_first_power) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    const uint64_t off = srs_order - claimed_len - trailing_first_power;
    if (off > g2_trailing->n || claimed_len > g2_trailing->n - off) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (n > g1_srs->n || n > g2_srs->n) return KZG_ERR_POLY_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (count == 0) return KZG_OK;
    if (n == 0) {
        memset(out_commitments_xy, 0, count * 64); memset(out_length_commitments, 0, count * 128); memset(out_length_proofs, 0, count * 128);
        return KZG_OK;
    }
    const void* d_scalars;
    int32_t rc = stage_scalars_g2(ctx, coeffs_mont, count * n, &d_scalars);     // the one upload: every MSM of every blob reads it
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                          // (the G1 launches run on the slots' streams)
    rc = commit_batch_device(ctx, g1_srs, d_scalars, n, count, out_commitments_xy, nullptr);
    if (rc != KZG_OK) return rc;
    const uint4* pts[2] = {g2_srs->d_points, g2_trailing->d_points + 8 * off};
    uint64_t* outs[2] = {out_length_commitments, out_length_proofs};
    return g2_msm_batch_run(ctx, pts, 2, d_scalars, n, count, outs, nullptr);    // per group: one digit pass and sort, both base sets in every launch
}

int32_t kzg_ctx_set_g2_batch_group(kzg_ctx* ctx, uint32_t max_blobs) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->g2_batch_group = max_blobs;
    return KZG_OK;
}

int32_t kzg_msm_g2_batch_info(size_t n, uint32_t nb, size_t count, uint32_t max_blobs, kzg_g2_batch_info* out) {
    if (!out || (nb != 1 && nb != 2)) return KZG_ERR_INVALID_ARG;
    { const int32_t rc = g2_batch_size_check(n, count); if (rc != KZG_OK) return rc; }
    *out = kzg_g2_batch_info{};
    if (n == 0 || count == 0) return KZG_OK;
    const uint32_t wave_slots = 256 * 4 * G2_ACC_WAVES;                  // a 256-CU device (what kzg_ctx_create finds on an MI355X)
    const bool batched = g2_batch_shares(n, nb);
    out->batched = batched ? 1 : 0;
    out->blobs_per_group = batched ? g2_batch_group(n, nb, count, max_blobs) : 1;
    out->groups = (count + out->blobs_per_group - 1) / out->blobs_per_group;
    // the first launch: above the launch cap, of the first G2MSM_MAX_LAUNCH scalars of one blob
    const G2Plan p = g2_make_plan(std::min<size_t>(n, G2MSM_MAX_LAUNCH), nb, out->blobs_per_group, wave_slots);
    out->entries = p.entries(); out->workspace_bytes = p.workspace_bytes;
    out->c = (uint32_t)p.c; out->W = (uint32_t)p.W; out->G = p.G; out->nl = p.nl; out->seg = p.seg;
    out->sort_small = p.sort.sort_small ? 1 : 0; out->scan1 = p.G <= SCAN1_MAX ? 1 : 0; out->launches = p.launches;
    return KZG_OK;
}

int32_t kzg_verify_length_proof(const uint64_t commitment_xy[8], const uint64_t length_commitment[16], const uint64_t length_proof[16],
                                const uint64_t g1_tau_shift_xy[8], int32_t* out_ok) {
    if (!commitment_xy || !length_commitment || !length_proof || !g1_tau_shift_xy || !out_ok) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    const G1 c = g1_from_wire(commitment_xy), shift = g1_from_wire(g1_tau_shift_xy);
    const G2 c2 = g2_from_wire(length_commitment), pi2 = g2_from_wire(length_proof);
    if (!g1_on_curve(c) || !g1_on_curve(shift)) return KZG_ERR_G1_NOT_ON_CURVE;
    if (!g2_on_curve(c2) || !g2_on_curve(pi2)) return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    G1 g1; g1.x = FQ_ONE; g1.y = FQ_TWO; g1.inf = false;
    const G2 g2 = g2_generator();
    // e(C, G2) = e(G1, C2): the two commitments hold the same polynomial; e([tau^(N-d)]_1, C2) = e(G1, pi2): pi2 is its shift by N - d
    *out_ok = pairings_verify(c, g2, g1, c2) && pairings_verify(shift, c2, g1, pi2) ? 1 : 0;
    return KZG_OK;
}

// ---- batches of blob headers ---------------------------------------------------------------------------------------------------
int32_t kzg_pairings_product_verify(const uint64_t* g1s_xy, const uint64_t* g2s, size_t count, int32_t* out_ok) {
    if (!out_ok || (count && (!g1s_xy || !g2s)) || count > ((size_t)1 << 30)) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    std::vector<G1> ps(count);
    std::vector<G2> qs(count);
    for (size_t k = 0; k < count; ++k) { ps[k] = g1_from_wire(g1s_xy + 8 * k); if (!g1_on_curve(ps[k])) return KZG_ERR_G1_NOT_ON_CURVE; }
    for (size_t k = 0; k < count; ++k) { qs[k] = g2_from_wire(g2s + 16 * k); if (!g2_on_curve(qs[k])) return KZG_ERR_G2_TAU_NOT_ON_CURVE; }
    *out_ok = pairings_product_is_one(ps.data(), qs.data(), (int)count, host_parallel_for) ? 1 : 0;
    return KZG_OK;
}

int32_t kzg_g2_check_subgroup(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n_points, uint64_t* bad_index) {
    if (!ctx || (n_points && !g2_mont)) return KZG_ERR_INVALID_ARG;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n_points == 0) return KZG_OK;
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_points * 128));
    int64_t off_twist = -1, outside = -1;
    int32_t rc = g2_upload_points(ctx, g2_mont, n_points, ctx->msm.bases.as<uint4>(), &off_twist);
    if (rc != KZG_OK) return rc;
    // the chain has no meaning off the twist: the points in front of the first such point are tested, and the smaller index is reported
    rc = g2_subgroup_check(ctx, ctx->msm.bases.as<uint4>(), off_twist >= 0 ? (size_t)off_twist : n_points, &outside);
    if (rc != KZG_OK) return rc;
    const int64_t bad = outside >= 0 ? outside : off_twist;
    if (bad < 0) return KZG_OK;
    if (bad_index) *bad_index = (uint64_t)bad;
    ctx->last_error = "kzg_g2_check_subgroup: point " + std::to_string(bad) + (outside >= 0 ? " is not in the order-r subgroup" : " is not on the twist");
    return KZG_ERR_NOT_ON_CURVE;
}

int32_t kzg_compute_header_batch_weights(const uint64_t* commitments_xy, const uint64_t* length_commitments, const uint64_t* length_proofs,
                                         const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens,
                                         const uint64_t* g1_tau_shifts_xy, size_t n_shifts, uint64_t* out_weights_mont) {
    if (!out_weights_mont) return KZG_ERR_INVALID_ARG;
    if (count && (!commitments_xy || !length_commitments || !length_proofs || !claimed_lens)) return KZG_ERR_INVALID_ARG;
    if (n_shifts && (!shift_lens || !g1_tau_shifts_xy)) return KZG_ERR_INVALID_ARG;
    kzg_host::header_batch_weights_host(commitments_xy, length_commitments, length_proofs, claimed_lens, count, shift_lens, g1_tau_shifts_xy, n_shifts,
                                        out_weights_mont, host_parallel_for);
    return KZG_OK;
}

int32_t kzg_verify_length_proof_batch(kzg_ctx* ctx, const uint64_t* commitments_xy, const uint64_t* length_commitments,
                                      const uint64_t* length_proofs, const uint64_t* claimed_lens, size_t count,
                                      const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                                      const uint64_t* weights_mont, int32_t* out_ok, uint64_t* bad_index) {
    HeaderStage st;
    bool empty = false;
    int32_t rc = header_batch_prefix("kzg_verify_length_proof_batch", ctx, !out_ok, commitments_xy, length_commitments, length_proofs, claimed_lens, count, shift_lens,
                                     g1_tau_shifts_xy, n_shifts, weights_mont, HeaderGrouping(), bad_index, &empty, &st);
    if (rc != KZG_OK) return rc;
    if (empty) { *out_ok = 1; return KZG_OK; }
    return header_verify_tail(ctx, st, commitments_xy, count, n_shifts, out_ok);
}

// ---- locating the bad headers of a rejected batch (g2batch.hip k_g2_locate_*, multilocate.hip k_locate_*<1>, host_header_locate.h) ----------
int32_t kzg_header_group_sums(kzg_ctx* ctx, const uint64_t* commitments_xy, const uint64_t* length_commitments, const uint64_t* length_proofs,
                              const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                              const uint64_t* weights_mont, const uint64_t* group_indices, size_t n_groups, uint64_t* out_u_xy, uint8_t* out_u_is_infinity,
                              uint64_t* out_w_g2, uint64_t* out_pi_g2, uint64_t* bad_index) {
    HeaderStage st;
    HeaderGrouping grp;
    grp.on = true; grp.group_indices = group_indices; grp.n_groups = n_groups;
    bool empty = false;
    const bool out_null = n_groups && (!out_u_xy || !out_u_is_infinity || !out_pi_g2 || (n_shifts && !out_w_g2));
    int32_t rc = header_batch_prefix("kzg_header_group_sums", ctx, out_null, commitments_xy, length_commitments, length_proofs, claimed_lens, count, shift_lens,
                                     g1_tau_shifts_xy, n_shifts, weights_mont, grp, bad_index, &empty, &st);
    if (rc != KZG_OK) return rc;
    HeaderGroupSums gs;
    if (!empty) {
        rc = header_group_sums_core(ctx, st, commitments_xy, count, n_shifts, group_indices, n_groups, &gs);
        if (rc != KZG_OK) return rc;
        st.lk.unlock();
    }
    if (n_groups) {                                                  // an empty group, an unclaimed class: identities
        memset(out_u_xy, 0, n_groups * 64);
        memset(out_u_is_infinity, 1, n_groups);
        if (n_shifts) memset(out_w_g2, 0, n_groups * n_shifts * 128);
        memset(out_pi_g2, 0, n_groups * 128);
    }
    const size_t S = gs.g1_plan.segs.size(), per = 256;
    std::vector<uint64_t> xy(8 * S);
    host_parallel_for((S + per - 1) / per, [&](size_t c) {
        const size_t a = c * per, b = std::min(S, (c + 1) * per);
        kzg_host::xyzz_batch_to_affine(gs.u.data() + a, b - a, xy.data() + 8 * a);
    });
    for (size_t j = 0; j < S; ++j) {
        memcpy(out_u_xy + 8 * (size_t)gs.g1_plan.segs[j], xy.data() + 8 * j, 64);
        out_u_is_infinity[gs.g1_plan.segs[j]] = kzg_host::is_inf(gs.u[j]) ? 1 : 0;
    }
    const size_t n_w = n_groups * n_shifts;                          // a key below it is g n_shifts + s: the row of W_{g,s} in out_w_g2
    for (size_t j = 0; j < gs.g2_plan.segs.size(); ++j) {
        const size_t key = gs.g2_plan.segs[j];
        memcpy(key < n_w ? out_w_g2 + 16 * key : out_pi_g2 + 16 * (key - n_w), gs.q.data() + 16 * j, 128);
    }
    return KZG_OK;
}

int32_t kzg_verify_length_proof_batch_locate(kzg_ctx* ctx, const uint64_t* commitments_xy, const uint64_t* length_commitments, const uint64_t* length_proofs,
                                             const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy,
                                             size_t n_shifts, const uint64_t* weights_mont, const uint64_t* group_indices, size_t n_groups,
                                             uint8_t* out_group_ok, size_t* out_bad_groups, size_t* out_pairing_checks, uint64_t* bad_index) {
    HeaderStage st;
    HeaderGrouping grp;
    grp.on = true; grp.group_indices = group_indices; grp.n_groups = n_groups;
    bool empty = false;
    int32_t rc = header_batch_prefix("kzg_verify_length_proof_batch_locate", ctx, !out_bad_groups || (n_groups && !out_group_ok), commitments_xy, length_commitments,
                                     length_proofs, claimed_lens, count, shift_lens, g1_tau_shifts_xy, n_shifts, weights_mont, grp, bad_index, &empty, &st);
    if (rc != KZG_OK) return rc;
    if (empty) {                                                     // nothing to refuse: no device work, no pairing
        if (n_groups) memset(out_group_ok, 1, n_groups);
        *out_bad_groups = 0;
        if (out_pairing_checks) *out_pairing_checks = 0;
        return KZG_OK;
    }
    return header_locate_tail(ctx, st, commitments_xy, count, n_shifts, group_indices, n_groups, out_group_ok, out_bad_groups, out_pairing_checks);
}

// ---- blob headers in their serialized form (headerbytes.hip, host_header_bytes.h) ----------------------------------------------------------
int32_t kzg_header_items_encode_be(const uint64_t* commitments_xy, const uint64_t* length_commitments, const uint64_t* length_proofs, size_t count,
                                   uint8_t* out_commitments_be, uint8_t* out_length_commitments_be, uint8_t* out_length_proofs_be) {
    if ((commitments_xy == nullptr) != (out_commitments_be == nullptr) || (length_commitments == nullptr) != (out_length_commitments_be == nullptr) ||
        (length_proofs == nullptr) != (out_length_proofs_be == nullptr))
        return KZG_ERR_INVALID_ARG;
    if (count && !commitments_xy && !length_commitments && !length_proofs) return KZG_ERR_INVALID_ARG;
    if (count > kzg::HEADER_MAX_COUNT) return KZG_ERR_TOO_LARGE;
    std::atomic<int> bad{0};
    const size_t per = 256, jobs = (count + per - 1) / per;
    host_parallel_for(jobs, [&](size_t j) {
        for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
            bool ok = true;
            if (commitments_xy) ok = kzg_host::g1_encode_be(commitments_xy + 8 * i, out_commitments_be + 32 * i) && ok;
            if (length_commitments) ok = kzg_host::g2_encode_be(length_commitments + 16 * i, out_length_commitments_be + 64 * i) && ok;
            if (length_proofs) ok = kzg_host::g2_encode_be(length_proofs + 16 * i, out_length_proofs_be + 64 * i) && ok;
            if (!ok) bad.store(1, std::memory_order_relaxed);
        }
    });
    return bad.load() ? KZG_ERR_INVALID_ARG : KZG_OK;
}

int32_t kzg_header_items_decode_be(kzg_ctx* ctx, const uint8_t* commitments_be, const uint8_t* length_commitments_be, const uint8_t* length_proofs_be, size_t count,
                                   uint64_t* out_commitments_xy, uint64_t* out_length_commitments, uint64_t* out_length_proofs, uint64_t* bad_index,
                                   int32_t* bad_array) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (count && (!commitments_be || !length_commitments_be || !length_proofs_be || !out_commitments_xy || !out_length_commitments || !out_length_proofs))
        return KZG_ERR_INVALID_ARG;
    if (count > kzg::HEADER_MAX_COUNT) return KZG_ERR_TOO_LARGE;
    if (count == 0) return KZG_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(2 * count * 128));
    KZG_HIP_TRY(ctx, ctx->ml[5].reserve(count * 65));                                   // wire commitments | identity bytes
    HeaderBytesDecode job;
    job.commitments_be = commitments_be; job.length_commitments_be = length_commitments_be; job.length_proofs_be = length_proofs_be;
    job.count = count;
    job.wire = true;
    job.d_commitments = ctx->ml[5].as<uint4>();
    job.d_commitments_inf = ctx->ml[5].as<uint8_t>() + count * 64;
    job.d_g2 = ctx->msm.bases.as<uint4>();
    int32_t rc = header_bytes_decode(ctx, &job);
    if (rc != KZG_OK) return rc;
    rc = header_bytes_status(ctx, "kzg_header_items_decode_be", job, bad_index, bad_array);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_commitments_xy, job.d_commitments, count * 64, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_length_commitments, job.d_g2, count * 128, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_length_proofs, job.d_g2 + 8 * count, count * 128, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

int32_t kzg_verify_length_proof_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments_be, const uint8_t* length_commitments_be, const uint8_t* length_proofs_be,
                                            const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                                            const uint64_t* weights_mont, int32_t* out_ok, uint64_t* out_weights_mont, uint64_t* bad_index, int32_t* bad_array) {
    HeaderStage st;
    bool empty = false;
    int32_t rc = header_batch_prefix_bytes("kzg_verify_length_proof_batch_bytes", ctx, !out_ok, commitments_be, length_commitments_be, length_proofs_be, claimed_lens, count,
                                           shift_lens, g1_tau_shifts_xy, n_shifts, weights_mont, HeaderGrouping(), bad_index, bad_array, &empty, &st);
    if (rc != KZG_OK) return rc;
    if (empty) { *out_ok = 1; return KZG_OK; }
    rc = header_verify_tail(ctx, st, nullptr, count, n_shifts, out_ok);
    if (rc == KZG_OK && out_weights_mont) memcpy(out_weights_mont, st.weights, (count + 1) * 32);
    return rc;
}

int32_t kzg_verify_length_proof_batch_locate_bytes(kzg_ctx* ctx, const uint8_t* commitments_be, const uint8_t* length_commitments_be, const uint8_t* length_proofs_be,
                                                   const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy,
                                                   size_t n_shifts, const uint64_t* weights_mont, const uint64_t* group_indices, size_t n_groups,
                                                   uint8_t* out_group_ok, size_t* out_bad_groups, size_t* out_pairing_checks, uint64_t* bad_index, int32_t* bad_array) {
    HeaderStage st;
    HeaderGrouping grp;
    grp.on = true; grp.group_indices = group_indices; grp.n_groups = n_groups;
    bool empty = false;
    int32_t rc = header_batch_prefix_bytes("kzg_verify_length_proof_batch_locate_bytes", ctx, !out_bad_groups || (n_groups && !out_group_ok), commitments_be,
                                           length_commitments_be, length_proofs_be, claimed_lens, count, shift_lens, g1_tau_shifts_xy, n_shifts, weights_mont, grp,
                                           bad_index, bad_array, &empty, &st);
    if (rc != KZG_OK) return rc;
    if (empty) {                                                     // nothing to refuse: no device work, no pairing
        if (n_groups) memset(out_group_ok, 1, n_groups);
        *out_bad_groups = 0;
        if (out_pairing_checks) *out_pairing_checks = 0;
        return KZG_OK;
    }
    return header_locate_tail(ctx, st, nullptr, count, n_shifts, group_indices, n_groups, out_group_ok, out_bad_groups, out_pairing_checks);
}

int32_t kzg_g2_decompress_be(const uint8_t* bytes, size_t n_points, uint64_t* out_g2_mont, uint64_t* bad_index) {
    if ((n_points && (!bytes || !out_g2_mont))) return KZG_ERR_INVALID_ARG;
    std::atomic<uint64_t> first_bad{UINT64_MAX};
    std::vector<int32_t> status(n_points, KZG_OK);
    host_parallel_for(n_points, [&](size_t i) {
        kzg_host::G2 p;
        status[i] = kzg_host::g2_decompress_be(bytes + 64 * i, p);
        if (status[i] == KZG_OK) { kzg_host::g2_to_wire(p, out_g2_mont + 16 * i); return; }
        uint64_t cur = first_bad.load();
        while (i < cur && !first_bad.compare_exchange_weak(cur, (uint64_t)i)) {}
    });
    const uint64_t bad = first_bad.load();
    if (bad == UINT64_MAX) return KZG_OK;
    if (bad_index) *bad_index = bad;
    return status[bad];
}

int32_t kzg_g2_decompress_be_device(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, uint32_t flags, uint64_t* out_g2_mont, uint64_t* bad_index) {
    if (!ctx || (n_points && (!bytes || !out_g2_mont)) || (flags & ~(KZG_G2_CHECK_SUBGROUP | KZG_G2_REJECT_GENERATOR))) return KZG_ERR_INVALID_ARG;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    uint32_t bad = 0xFFFFFFFFu;
    const int32_t rc = g2_decompress_run(ctx, bytes, n_points, flags, nullptr, out_g2_mont, &bad);
    if (rc != KZG_OK) return rc;
    return g2_decode_status(ctx, "kzg_g2_decompress_be_device", bad, bad_index);
}

int32_t kzg_g2srs_load_compressed_be(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_g2srs** out, uint64_t* bad_index) {
    if (!ctx || !out || (n_points && !bytes)) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    int32_t rc;
    kzg_g2srs* s = new_handle(ctx, n_points, &rc);
    if (!s) return rc;
    uint32_t bad = 0xFFFFFFFFu;
    rc = g2_decompress_run(ctx, bytes, n_points, KZG_G2_CHECK_SUBGROUP, s->d_points, nullptr, &bad);     // the generator is [tau^0]_2 of a file
    if (rc == KZG_OK) rc = g2_decode_status(ctx, "kzg_g2srs_load_compressed_be", bad, bad_index);
    if (rc != KZG_OK) { drop_handle(s); return rc; }
    *out = s;
    return KZG_OK;
}

}  // extern "C"

KZG_BOUND_CHECK_EXPORTS(capi_g2)
