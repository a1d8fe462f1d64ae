// capi_verify.hip — the verifier surface of the C-ABI: the pairing checks (O(1) host pairing, the data-parallel part on the GPU), the
// batch verifier of blob proofs (verifier/src/batch.rs) with its transcript entries, rows of SHA-256, erasure decoding.
// (The verifiers of FK20 coset proofs: capi_coset.hip.)
#include "engine.h"
#include "host_curve.h"
#include "host_pairing.h"
#include "host_sha256.h"
#include "host_fiat_shamir.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

using namespace kzg;
using kzg_host::blob_padded_len;
using kzg_host::r_powers_host;

// ---- verifier surface: O(1) host pairing, data-parallel part on the GPU ---------------------------------------------
namespace kzg {
bool load_g2_tau(const uint64_t* g2_tau_mont, kzg_host::G2* out) {
    *out = g2_tau_mont ? kzg_host::g2_from_wire(g2_tau_mont) : kzg_host::g2_tau_mainnet();
    return kzg_host::g2_on_curve(*out);
}

// helpers::pairings_verify for the batch verifiers: the two Miller loops on the persistent host pool (a parked worker wakes in ~20 us; host_pairing.h's own
// form starts a std::thread per call), then the one final exponentiation.  Same Fq12 values, bit for bit.
bool pairings_verify_pooled(const kzg_host::G1& a1, const kzg_host::G2& a2, const kzg_host::G1& b1, const kzg_host::G2& b2) {
    using namespace kzg_host;
    G1 ps[2] = {a1, g1_neg(b1)};
    G2 qs[2] = {a2, b2};
    Fq12 f[2];
    bool bad[2] = {false, false};
    host_parallel_for(2, [&](size_t k) { f[k] = miller_ate_product(ps + k, qs + k, 1, &bad[k]); });
    if (bad[0] || bad[1]) return false;
    return fq12_is_one(final_exponentiation_x(mul(f[0], f[1])));
}
}  // namespace kzg

namespace {
int32_t verify_batch_core(kzg_ctx* ctx, const uint64_t* commitments_xy_mont, const uint64_t* zs_mont, const uint64_t* ys_mont,
                                 const uint64_t* proofs_xy_mont, const uint64_t* r_powers_mont, size_t n,
                                 const uint64_t* g2_tau_mont, int32_t* out_ok) {
    using namespace kzg_host;
    // batch.rs:203-210 (every commitment and proof on the curve) is checked on the GPU, on the points the MSM uploads anyway
    // (k_points_wire_to_device_checked: 2n curve equations cost the host 0.5 ms at n = 4096); the error order of the reference is
    // kept: a point off the curve is reported before a bad g2_tau (batch.rs:214-216).
    G2 g2_tau;
    const bool g2_ok = load_g2_tau(g2_tau_mont, &g2_tau);
    // scalars of the three linear combinations (batch.rs:228, :245, :246).  sum_i r^i (C_i - [y_i]G) is evaluated as
    // sum_i r^i C_i - [sum_i r^i y_i] G: the same group element with one fixed-base product instead of n.
    std::vector<uint64_t> bases(3 * n * 8), scalars(3 * n * 4);
    uint64_t s[4] = {0, 0, 0, 0};
    {
        // 2 n field products (0.15 ms at n = 4096 on one core): chunks on the host pool, one partial sum per chunk
        const size_t chunks = n >= 1024 ? 32 : 1, per = (n + chunks - 1) / chunks;
        std::vector<uint64_t> partial(4 * chunks, 0);
        auto body = [&](size_t c) {
            uint64_t acc[4] = {0, 0, 0, 0};
            for (size_t i = c * per; i < std::min(n, (c + 1) * per); ++i) {
                uint64_t t[4];
                fr_mul(r_powers_mont + 4 * i, zs_mont + 4 * i, scalars.data() + (n + i) * 4);      // r^i z_i
                fr_mul(r_powers_mont + 4 * i, ys_mont + 4 * i, t);
                fr_add(acc, t, acc);
            }
            memcpy(partial.data() + 4 * c, acc, 32);
        };
        if (chunks > 1) host_parallel_for(chunks, body); else body(0);
        for (size_t c = 0; c < chunks; ++c) fr_add(s, partial.data() + 4 * c, s);
    }
    if (n) {
        memcpy(bases.data(), proofs_xy_mont, n * 64);
        memcpy(bases.data() + n * 8, proofs_xy_mont, n * 64);
        memcpy(bases.data() + 2 * n * 8, commitments_xy_mont, n * 64);
        memcpy(scalars.data(), r_powers_mont, n * 32);
        memcpy(scalars.data() + 2 * n * 4, r_powers_mont, n * 32);
    }
    uint64_t sums[3 * 8];
    uint8_t infs[3];
    uint32_t off_curve = 0;
    const auto t_c0 = Clock::now();
    int32_t rc = msm_g1_batch_impl(ctx, bases.data(), scalars.data(), n, 3, sums, infs, &off_curve);
    const auto t_c1 = Clock::now();
    if (rc != KZG_OK) return rc;
    if (off_curve) return KZG_ERR_G1_NOT_ON_CURVE;
    if (!g2_ok) return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    G1 proof_lincomb = g1_from_wire(sums), proof_z_lincomb = g1_from_wire(sums + 8), c_lincomb = g1_from_wire(sums + 16);
    uint64_t s_int[4];
    fr_wire_to_canonical(s, s_int);
    G1 rhs = g1_add(g1_add(c_lincomb, g1_neg(g1_mul_generator(s_int))), proof_z_lincomb);   // batch.rs:249
    const auto t_c2 = Clock::now();
    *out_ok = pairings_verify_pooled(proof_lincomb, g2_tau, rhs, g2_generator()) ? 1 : 0;  // batch.rs:253-254
    if (opts().vb_trace) {
        fprintf(stderr, "  verify_batch_core n=%zu: three MSMs (upload, kernels, host Horner) %.3f ms, [s]G + point sums %.3f ms, pairing check %.3f ms\n", n, ms_between(t_c0, t_c1), ms_between(t_c1, t_c2),
                ms_between(t_c2, Clock::now()));
    }
    return KZG_OK;
}

// ---- batch verification end to end (verifier/src/batch.rs:16-69, :76-168; primitives/src/helpers.rs:613-662) ---------------------
constexpr size_t VB_GROUP_BYTES = (size_t)256 << 20;           // packed blob bytes per GPU round

// The data-parallel front end of verify_blob_kzg_proof_batch: z_i = compute_challenge(blob_i, C_i), y_i = p_i(z_i) for all n blobs.
// Transcripts: n independent SHA-256 streams on a pool of host threads (each also packs its blob into the pinned staging buffer);
// evaluations: two GPU launches for all blobs of up to 4096 elements (vbeval.hip k_vb_prep / k_vb_eval), the single-polynomial path
// for the rest.  `validated` = the caller has already checked every commitment (batch.rs:29-37); otherwise compute_challenge's own
// validate_g1_point (helpers.rs:413) is reported in blob order.
// commitments == nullptr: zs are INPUTS (kzg_evaluate_blobs_in_evaluation_form_batch), nothing is hashed.
int32_t challenges_and_evaluations(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* lens, const uint64_t* commitments, size_t n,
                                   bool validated, uint64_t* zs, uint64_t* ys) {
    using namespace kzg_host;
    // per-blob guards in the reference's order (helpers.rs:634-645): to_polynomial_eval_form (TOO_LARGE), compute_challenge
    // (validate_g1_point), evaluate_polynomial_in_evaluation_form -> calculate_roots_of_unity (ZERO_LENGTH)
    std::vector<int32_t> status(n, KZG_OK);
    std::vector<VbBlob> meta(n);
    std::vector<size_t> group_end;                            // blob index where each GPU round ends
    // (KZG_VB_GROUP_BYTES / KZG_VB_CHUNK_BYTES: staging granularity; tests shrink them so that small batches take the multi-round / multi-chunk paths)
    const size_t group_bytes = opts().vb_group_bytes ? opts().vb_group_bytes : VB_GROUP_BYTES;
    const size_t chunk_bytes = opts().vb_chunk_bytes ? opts().vb_chunk_bytes : ((size_t)16 << 20);
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t elems = (lens[i] + 31) / 32;
        if (lens[i] && !blobs[i]) return KZG_ERR_INVALID_ARG;
        if (elems > ((size_t)1 << 28)) { status[i] = KZG_ERR_TOO_LARGE; meta[i] = VbBlob{0, 0, 99}; continue; }
        const uint32_t lg = (uint32_t)__builtin_ctzll(kzg_host::next_pow2(elems));
        const bool batched = lens[i] != 0 && lg <= (uint32_t)VB_MAX_LOG;
        const size_t span = batched ? elems * 32 : 0;
        if (off && off + span > group_bytes) { group_end.push_back(i); off = 0; }
        meta[i] = VbBlob{(uint64_t)off, (uint32_t)(batched ? lens[i] : 0), batched ? lg : 99u};
        off += span;
    }
    group_end.push_back(n);
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    std::vector<uint8_t> fallback(n, 0);
    size_t g0 = 0;
    for (size_t g1 : group_end) {
        size_t bytes = 0;
        for (size_t i = g0; i < g1; ++i) if (meta[i].log_n != 99u) bytes = std::max(bytes, (size_t)meta[i].off + ((size_t)meta[i].len + 31) / 32 * 32);
        const size_t bytes_al = (bytes + 4095) / 4096 * 4096, small_bytes = (g1 - g0) * 48 + 4096;   // packed blobs | challenges + descriptors
        if (bytes_al + small_bytes > ctx->vb_pinned_bytes) {
            if (ctx->vb_pinned) { (void)hipHostFree(ctx->vb_pinned); ctx->vb_pinned = nullptr; ctx->vb_pinned_bytes = 0; }
            const size_t cap = bytes_al + bytes_al / 4 + 2 * small_bytes;
            KZG_HIP_TRY(ctx, hipHostMalloc(&ctx->vb_pinned, cap, hipHostMallocDefault));
            ctx->vb_pinned_bytes = cap;
        }
        uint8_t* stage = static_cast<uint8_t*>(ctx->vb_pinned);
        RoctxPhases phases;
        phases.begin("kzg:batch_verify:transcripts + pack (host threads) | uploads + evaluation kernels (GPU)");
        const auto t_hash0 = Clock::now();
        const size_t nb = g1 - g0;
        int32_t rc = vb_evaluate_setup(ctx, bytes, nb);
        if (rc != KZG_OK) return rc;
        // Chunks of ~16 MiB of packed bytes: the thread that finishes the LAST blob of a chunk enqueues the chunk's upload and its two
        // kernels, so the PCIe transfer and the evaluations run beside the hashing of the later blobs (3 ms of host work and 3 ms of
        // upload + kernels one after the other before).  The pool hands blobs out in index order, so chunks complete roughly in order.
        std::vector<size_t> chunk_of(nb), chunk_lo, chunk_hi;
        {
            size_t acc_bytes = 0;
            for (size_t k = 0; k < nb; ++k) {
                if (chunk_lo.empty() || acc_bytes >= chunk_bytes) { chunk_lo.push_back(k); chunk_hi.push_back(k); acc_bytes = 0; }
                chunk_of[k] = chunk_lo.size() - 1;
                chunk_hi.back() = k + 1;
                if (meta[g0 + k].log_n != 99u) acc_bytes += ((size_t)meta[g0 + k].len + 31) / 32 * 32;
            }
        }
        std::vector<std::atomic<uint32_t>> left(chunk_lo.size());
        for (size_t c = 0; c < chunk_lo.size(); ++c) left[c].store((uint32_t)(chunk_hi[c] - chunk_lo[c]));
        std::atomic<int32_t> enqueue_rc{KZG_OK};
        const bool trace_chunks = opts().vb_trace >= 2;
        std::vector<double> enq_at(chunk_lo.size(), 0.0), enq_took(chunk_lo.size(), 0.0);
        std::vector<hipEvent_t> chunk_ev(trace_chunks ? chunk_lo.size() : 0);
        hipEvent_t ev0 = nullptr;
        if (trace_chunks) { for (auto& e : chunk_ev) (void)hipEventCreate(&e); (void)hipEventCreate(&ev0); (void)hipEventRecord(ev0, ctx->stream); }
        // Pool jobs: PAIRS of blobs of one upload chunk with similar transcript lengths (sorted inside the chunk), so that the two SHA-256 streams of a
        // job run interleaved in one thread to the end (host_transcript.h: 1.5 x the single-stream rate); chunks stay in index order, so they still
        // complete -- and go up -- roughly in order.  A blob that is not hashed (bad status, no commitments) rides along as a job of its own.
        std::vector<std::pair<uint32_t, uint32_t>> jobs;                 // blob indices relative to g0; second = UINT32_MAX: a single
        jobs.reserve(nb / 2 + chunk_lo.size() + 1);
        {
            std::vector<uint32_t> order;
            for (size_t c = 0; c < chunk_lo.size(); ++c) {
                order.clear();
                for (size_t k = chunk_lo[c]; k < chunk_hi[c]; ++k) order.push_back((uint32_t)k);
                std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                    const size_t lx = lens[g0 + x], ly = lens[g0 + y];
                    return lx != ly ? lx > ly : x < y;
                });
                for (size_t q = 0; q < order.size(); q += 2)
                    jobs.emplace_back(order[q], q + 1 < order.size() && commitments ? order[q + 1] : UINT32_MAX);
                if (!commitments) for (size_t q = 1; q < order.size(); q += 2) jobs.emplace_back(order[q], UINT32_MAX);
            }
        }
        host_parallel_for(jobs.size(), [&](size_t jdx) {
            auto done = [&](size_t k) {
                const size_t c = chunk_of[k];
                if (left[c].fetch_sub(1, std::memory_order_acq_rel) == 1) {
                    const auto e0 = Clock::now();
                    const int32_t r = vb_evaluate_enqueue(ctx, stage, meta.data() + g0, nb, chunk_lo[c], chunk_hi[c], zs + 4 * g0, stage + bytes_al);
                    if (r != KZG_OK) enqueue_rc.store(r);
                    if (trace_chunks) {
                        (void)hipEventRecord(chunk_ev[c], ctx->stream);
                        enq_at[c] = ms_between(t_hash0, e0);
                        enq_took[c] = ms_between(e0, Clock::now());
                    }
                }
            };
            // per blob: guards in the reference's order, packing; returns the bytes to hash (nullptr: nothing to hash for this blob)
            auto prepare = [&](size_t k, G1& c) -> const uint8_t* {
                const size_t i = g0 + k;
                if (status[i] != KZG_OK) return nullptr;
                if (commitments) {
                    c = g1_from_wire(commitments + 8 * i);
                    if (!validated && !g1_on_curve(c)) { status[i] = KZG_ERR_G1_NOT_ON_CURVE; return nullptr; }
                }
                if (lens[i] == 0) { status[i] = KZG_ERR_ZERO_LENGTH; return nullptr; }
                const uint8_t* src = blobs[i];
                if (meta[i].log_n != 99u) {                       // pack (zero-filled to the 32-byte chunk) and hash the packed copy
                    uint8_t* dst = stage + meta[i].off;
                    const size_t span = (lens[i] + 31) / 32 * 32;
                    memcpy(dst, blobs[i], lens[i]);                   // (a probe build without this copy: 3.6-4.6 ms for the phase against 4.0-4.4 with it -- inside the noise)
                    if (span > lens[i]) memset(dst + lens[i], 0, span - lens[i]);
                    src = dst;
                }
                return commitments ? src : nullptr;
            };
            const size_t ka = jobs[jdx].first, kb = jobs[jdx].second;
            G1 ca, cb;
            const uint8_t* pa = prepare(ka, ca);
            const uint8_t* pb = kb != UINT32_MAX ? prepare(kb, cb) : nullptr;
            if (pa && pb) {
                Sha256 sa, sb;
                sha256_init(sa); sha256_init(sb);
                TranscriptPrefix ga(pa, lens[g0 + ka], blob_padded_len(lens[g0 + ka])), gb(pb, lens[g0 + kb], blob_padded_len(lens[g0 + kb]));
                sha256_absorb_x2(sa, ga, sb, gb);
                challenge_finish(sa, ca, zs + 4 * (g0 + ka));
                challenge_finish(sb, cb, zs + 4 * (g0 + kb));
            } else {
                for (int w = 0; w < 2; ++w) {
                    const uint8_t* p1 = w ? pb : pa;
                    if (!p1) continue;
                    const size_t k1 = w ? kb : ka;
                    Sha256 sh;
                    sha256_init(sh);
                    challenge_absorb_prefix(sh, p1, lens[g0 + k1], blob_padded_len(lens[g0 + k1]));
                    challenge_finish(sh, w ? cb : ca, zs + 4 * (g0 + k1));
                }
            }
            done(ka);
            if (kb != UINT32_MAX) done(kb);
        });
        const auto t_hash_done = Clock::now();
        rc = vb_evaluate_finish(ctx, nb, ys + 4 * g0, fallback.data() + g0);         // (also drains the stream before any early return below)
        if (trace_chunks) {
            for (size_t c = 0; c < chunk_lo.size(); ++c) {
                float gpu_ms = 0;
                (void)hipEventElapsedTime(&gpu_ms, ev0, chunk_ev[c]);
                fprintf(stderr, "    chunk %zu blobs [%zu, %zu): enqueued at %.3f ms (call took %.3f ms), done on the GPU %.3f ms after the first enqueue point\n", c, chunk_lo[c],
                        chunk_hi[c], enq_at[c], enq_took[c], gpu_ms);
                (void)hipEventDestroy(chunk_ev[c]);
            }
            (void)hipEventDestroy(ev0);
        }
        if (enqueue_rc.load() != KZG_OK) return enqueue_rc.load();
        if (rc != KZG_OK) return rc;
        for (size_t i = g0; i < g1; ++i) if (status[i] != KZG_OK) return status[i];      // the first failing blob, in order
        {
            const bool trace = opts().vb_trace != 0;
            if (trace)
                fprintf(stderr, "  blobs [%zu, %zu): %zu packed bytes in %zu chunks; transcripts + pack %.3f ms (%u host threads, uploads and kernels beside them), "
                        "the rest of the GPU work + D2H %.3f ms\n", g0, g1, bytes, chunk_lo.size(),
                        ms_between(t_hash0, t_hash_done), host_pool_threads(nb),
                        ms_between(t_hash_done, Clock::now()));
        }
        g0 = g1;
    }
    for (size_t i = 0; i < n; ++i) {                          // z on the domain, or more than 4096 elements: one polynomial at a time
        if (!fallback[i]) continue;
        const size_t np = blob_padded_len(lens[i]);
        PolySet& set = ctx->poly[0];
        void* d_evals = nullptr;
        int32_t rc = blob_to_fr_run(ctx, blobs[i], lens[i], np, &d_evals, ctx->stream, &set.c, &set.a);
        if (rc == KZG_OK) rc = proof_run(ctx, nullptr, nullptr, np, zs + 4 * i, nullptr, nullptr, ys + 4 * i, false, 0, nullptr);
        if (rc != KZG_OK) return rc;
    }
    return KZG_OK;
}

}  // namespace

extern "C" {

int32_t kzg_g2_generator(uint64_t out_g2_mont[16]) {
    if (!out_g2_mont) return KZG_ERR_INVALID_ARG;
    kzg_host::g2_to_wire(kzg_host::g2_generator(), out_g2_mont);
    return KZG_OK;
}
int32_t kzg_g2_tau_mainnet(uint64_t out_g2_mont[16]) {
    if (!out_g2_mont) return KZG_ERR_INVALID_ARG;
    kzg_host::g2_to_wire(kzg_host::g2_tau_mainnet(), out_g2_mont);
    return KZG_OK;
}
int32_t kzg_g2_mul_generator(const uint64_t scalar_mont[4], uint64_t out_g2_mont[16]) {
    if (!scalar_mont || !out_g2_mont) return KZG_ERR_INVALID_ARG;
    uint64_t k[4];
    kzg_host::fr_wire_to_canonical(scalar_mont, k);
    kzg_host::g2_to_wire(kzg_host::g2_mul_generator(k), out_g2_mont);
    return KZG_OK;
}

int32_t kzg_g2_is_on_curve(const uint64_t g2_mont[16], int32_t* out_on_curve) {
    if (!g2_mont || !out_on_curve) return KZG_ERR_INVALID_ARG;
    *out_on_curve = kzg_host::g2_on_curve(kzg_host::g2_from_wire(g2_mont)) ? 1 : 0;
    return KZG_OK;
}

int32_t kzg_validate_g2_point(const uint64_t g2_mont[16], int32_t* out_reason) {
    if (!g2_mont || !out_reason) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    const G2 p = g2_from_wire(g2_mont);
    *out_reason = 0;
    if (!g2_on_curve(p)) { *out_reason = 1; return KZG_OK; }                               // helpers.rs:741-745
    if (p.inf) { *out_reason = 2; return KZG_OK; }                                          // :747-751
    if (!g2_mul(p, FR_MODULUS_WORDS).inf) { *out_reason = 3; return KZG_OK; }                          // :753-757: [r] P = O <=> P in the order-r subgroup of the twist
    const G2 g = g2_generator();
    if (eq(p.x, g.x) && eq(p.y, g.y)) { *out_reason = 4; return KZG_OK; }                   // :759-763
    return KZG_OK;
}

int32_t kzg_pairings_verify(const uint64_t a1_xy_mont[8], const uint64_t a2_g2_mont[16], const uint64_t b1_xy_mont[8],
                            const uint64_t b2_g2_mont[16], int32_t* out_ok) {
    if (!a1_xy_mont || !a2_g2_mont || !b1_xy_mont || !b2_g2_mont || !out_ok) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    G1 a1 = g1_from_wire(a1_xy_mont), b1 = g1_from_wire(b1_xy_mont);
    G2 a2 = g2_from_wire(a2_g2_mont), b2 = g2_from_wire(b2_g2_mont);
    if (!g1_on_curve(a1) || !g1_on_curve(b1)) return KZG_ERR_G1_NOT_ON_CURVE;
    if (!g2_on_curve(a2) || !g2_on_curve(b2)) return KZG_ERR_INVALID_ARG;
    *out_ok = pairings_verify(a1, a2, b1, b2) ? 1 : 0;
    return KZG_OK;
}

int32_t kzg_verify_proof(const uint64_t commitment_xy_mont[8], const uint64_t proof_xy_mont[8], const uint64_t value_mont[4],
                         const uint64_t z_mont[4], const uint64_t* g2_tau_mont, int32_t* out_ok) {
    if (!commitment_xy_mont || !proof_xy_mont || !value_mont || !z_mont || !out_ok) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    G1 commitment = g1_from_wire(commitment_xy_mont), proof = g1_from_wire(proof_xy_mont);
    if (!g1_on_curve(commitment) || !g1_on_curve(proof)) return KZG_ERR_G1_NOT_ON_CURVE;   // verify.rs:18,22 (G1 has cofactor 1)
    G2 g2_tau;
    if (!load_g2_tau(g2_tau_mont, &g2_tau)) return KZG_ERR_G2_TAU_NOT_ON_CURVE;            // verify.rs:29-33
    uint64_t y[4], z[4];
    fr_wire_to_canonical(value_mont, y);
    fr_wire_to_canonical(z_mont, z);
    G1 commit_minus_value = g1_add(commitment, g1_neg(g1_mul_generator(y)));               // verify.rs:37-42 (fixed-base tables)
    G2 x_minus_z = g2_add(g2_tau, g2_neg(g2_mul_generator(z)));                            // verify.rs:46-51
    if (x_minus_z.inf) return KZG_ERR_TAU_EQUALS_Z;                                        // verify.rs:56-60
    *out_ok = pairings_verify(commit_minus_value, g2_generator(), proof, x_minus_z) ? 1 : 0;   // verify.rs:66-71
    return KZG_OK;
}

int32_t kzg_verify_kzg_proof_batch(kzg_ctx* ctx, const uint64_t* commitments_xy_mont, const uint64_t* zs_mont, const uint64_t* ys_mont,
                                   const uint64_t* proofs_xy_mont, const uint64_t* r_powers_mont, size_t n,
                                   const uint64_t* g2_tau_mont, int32_t* out_ok) {
    if (!ctx || !out_ok) return KZG_ERR_INVALID_ARG;
    if (n && (!commitments_xy_mont || !zs_mont || !ys_mont || !proofs_xy_mont || !r_powers_mont)) return KZG_ERR_INVALID_ARG;
    return verify_batch_core(ctx, commitments_xy_mont, zs_mont, ys_mont, proofs_xy_mont, r_powers_mont, n, g2_tau_mont, out_ok);
}

int32_t kzg_compute_challenges_and_evaluate_polynomial(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* blob_lens,
                                                       const uint64_t* commitments_xy_mont, size_t n, uint64_t* out_zs_mont, uint64_t* out_ys_mont) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (n == 0) return KZG_OK;
    if (!blobs || !blob_lens || !commitments_xy_mont || !out_zs_mont || !out_ys_mont) return KZG_ERR_INVALID_ARG;
    return challenges_and_evaluations(ctx, blobs, blob_lens, commitments_xy_mont, n, false, out_zs_mont, out_ys_mont);
}

int32_t kzg_evaluate_blobs_in_evaluation_form_batch(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* blob_lens, const uint64_t* zs_mont,
                                                    size_t n, uint64_t* out_ys_mont) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (n == 0) return KZG_OK;
    if (!blobs || !blob_lens || !zs_mont || !out_ys_mont) return KZG_ERR_INVALID_ARG;
    return challenges_and_evaluations(ctx, blobs, blob_lens, nullptr, n, true, const_cast<uint64_t*>(zs_mont), out_ys_mont);
}

int32_t kzg_compute_r_powers(const uint64_t* commitments_xy_mont, const uint64_t* zs_mont, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont,
                             const uint64_t* blobs_as_field_elements_length, size_t n, uint64_t* out_r_powers_mont) {
    if (n == 0) return KZG_OK;
    if (!commitments_xy_mont || !zs_mont || !ys_mont || !proofs_xy_mont || !blobs_as_field_elements_length || !out_r_powers_mont) return KZG_ERR_INVALID_ARG;
    r_powers_host(commitments_xy_mont, zs_mont, ys_mont, proofs_xy_mont, blobs_as_field_elements_length, n, out_r_powers_mont, host_parallel_for);
    return KZG_OK;
}

int32_t kzg_sha256_rows(kzg_ctx* ctx, const uint8_t* msgs, size_t row_len, size_t count, uint8_t* out_digests) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (count == 0) return KZG_OK;
    if (!out_digests || (row_len && !msgs)) return KZG_ERR_INVALID_ARG;
    if (count > ((size_t)1 << 28) || (row_len && count > ((size_t)1 << 31) / row_len)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return sha256_rows_run(ctx, msgs, row_len, count, out_digests);
}

// erasure decoding: every check on the host before the context is touched (host_recover.h), then recover.hip
int32_t kzg_recover_from_cosets(kzg_ctx* ctx, const uint64_t* ys_mont, const uint64_t* coset_indices, size_t count, size_t n, size_t chunk_len,
                                size_t degree_bound, int32_t eval_form, uint64_t* out_poly_mont, int32_t* out_consistent) {
    RecoverPlan plan;
    int32_t rc = recover_plan(!ctx || !ys_mont || !coset_indices || !out_poly_mont, coset_indices, count, n, chunk_len, degree_bound, &plan);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t consistent = 0;
    rc = recover_run(ctx, plan, ys_mont, eval_form != 0, out_poly_mont, &consistent);
    if (rc != KZG_OK) return rc;
    if (out_consistent) *out_consistent = consistent;
    return KZG_OK;
}

// the same for many blobs of one shape: the checks (host_recover.h), the plan under the context's budget, then recover.hip group by group
int32_t kzg_recover_from_cosets_batch(kzg_ctx* ctx, const uint64_t* ys_mont, const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count,
                                      size_t n, size_t chunk_len, size_t degree_bound, int32_t eval_form, size_t out_len, uint64_t* out_polys_mont,
                                      int32_t* out_consistent) {
    int32_t rc = recover_batch_check(!ctx || !ys_mont || !coset_indices || !out_polys_mont, coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound,
                                     eval_form != 0, out_len);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RecoverBatchPlan plan;
    recover_batch_plan(coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound, eval_form != 0, out_len, ctx->recover_group_bytes, &plan);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    RecoverIo io;
    io.ys = ys_mont; io.out = out_polys_mont; io.consistent = out_consistent;
    return recover_run_batch(ctx, plan, io);
}

int32_t kzg_ctx_set_recover_group_bytes(kzg_ctx* ctx, size_t bytes) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->recover_group_bytes = bytes;
    return KZG_OK;
}

int32_t kzg_recover_batch_info(size_t blobs, size_t count, size_t n, size_t chunk_len, size_t out_len, size_t group_bytes, kzg_recover_batch_info_t* out) {
    const int32_t rc = recover_batch_info_check(!out, blobs, count, n, chunk_len, out_len);
    if (rc != KZG_OK) return rc;
    const RecoverBatchGroups g = recover_batch_groups(blobs, count, n, chunk_len, group_bytes);
    *out = kzg_recover_batch_info_t{};
    out->blobs_per_group = g.group;
    out->groups = g.n_groups;
    out->group_bytes = g.group_bytes;
    out->blob_bytes = g.blob_bytes;
    return KZG_OK;
}

// verify::verify_blob_kzg_proof (verifier/src/verify.rs:76-98) in one call: validate both points, z = compute_challenge(blob, commitment),
// y = p(z) (one batched-evaluation launch of one blob), then verify::verify_proof (verify.rs:10-72) on the host.
int32_t kzg_verify_blob_kzg_proof(kzg_ctx* ctx, const uint8_t* blob_bytes, size_t len, const uint64_t commitment_xy_mont[8],
                                  const uint64_t proof_xy_mont[8], const uint64_t* g2_tau_mont, int32_t* out_ok) {
    if (!ctx || !out_ok || !commitment_xy_mont || !proof_xy_mont || (len && !blob_bytes)) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    if (!g1_on_curve(g1_from_wire(commitment_xy_mont)) || !g1_on_curve(g1_from_wire(proof_xy_mont))) return KZG_ERR_G1_NOT_ON_CURVE;   // verify.rs:82,85
    uint64_t z[4], y[4];
    const uint8_t* blobs[1] = {blob_bytes};
    const size_t lens[1] = {len};
    int32_t rc = challenges_and_evaluations(ctx, blobs, lens, commitment_xy_mont, 1, true, z, y);     // verify.rs:88-94
    if (rc != KZG_OK) return rc;
    return kzg_verify_proof(commitment_xy_mont, proof_xy_mont, y, z, g2_tau_mont, out_ok);            // verify.rs:97
}

int32_t kzg_verify_blob_kzg_proof_batch(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* blob_lens, const uint64_t* commitments_xy_mont,
                                        const uint64_t* proofs_xy_mont, size_t n, const uint64_t* g2_tau_mont, int32_t* out_ok) {
    if (!ctx || !out_ok) return KZG_ERR_INVALID_ARG;
    if (n && (!blobs || !blob_lens || !commitments_xy_mont || !proofs_xy_mont)) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    const bool trace = opts().vb_trace != 0;                                                                   // phase times on stderr
    const auto t_start = Clock::now();
    // batch.rs:29-37: every commitment, then every proof, on the curve (cofactor 1: no subgroup check to make) -- before anything else
    {
        std::atomic<int> bad{0};
        const size_t per = 128, jobs = (2 * n + per - 1) / per;           // (one pool job per point was 8 192 contended counter increments: 0.3 ms for 0.05 ms of work)
        host_parallel_for(jobs, [&](size_t j) {
            for (size_t k = j * per; k < std::min(2 * n, (j + 1) * per); ++k) {
                const uint64_t* p = k < n ? commitments_xy_mont + 8 * k : proofs_xy_mont + 8 * (k - n);
                if (!g1_on_curve(g1_from_wire(p))) bad.store(1, std::memory_order_relaxed);
            }
        });
        if (bad.load()) return KZG_ERR_G1_NOT_ON_CURVE;
    }
    const auto t_valid = Clock::now();
    std::vector<uint64_t> zs(4 * n), ys(4 * n), rp(4 * n), lens_elems(n);
    auto t_eval = t_valid, t_rp = t_valid;
    if (n) {
        int32_t rc = challenges_and_evaluations(ctx, blobs, blob_lens, commitments_xy_mont, n, true, zs.data(), ys.data());   // batch.rs:43-44
        if (rc != KZG_OK) return rc;
        t_eval = Clock::now();
        for (size_t i = 0; i < n; ++i) lens_elems[i] = (uint64_t)blob_padded_len(blob_lens[i]);                              // batch.rs:48-54
        RoctxRange range_rp("kzg:batch_verify:r_powers (host)");
        r_powers_host(commitments_xy_mont, zs.data(), ys.data(), proofs_xy_mont, lens_elems.data(), n, rp.data(), host_parallel_for);           // batch.rs:222
        t_rp = Clock::now();
    }
    RoctxRange range_core("kzg:batch_verify:lincombs (GPU) + pairing (host)");
    const int32_t rc = verify_batch_core(ctx, commitments_xy_mont, zs.data(), ys.data(), proofs_xy_mont, rp.data(), n, g2_tau_mont, out_ok);   // batch.rs:62-68
    if (trace)
        fprintf(stderr, "kzg_verify_blob_kzg_proof_batch n=%zu: point validation %.3f ms, challenges + evaluations %.3f ms, r_powers %.3f ms, lincombs + pairing %.3f ms, call %.3f ms\n",
                n, ms_between(t_start, t_valid), ms_between(t_valid, t_eval), ms_between(t_eval, t_rp), ms_between(t_rp, Clock::now()), ms_between(t_start, Clock::now()));
    return rc;
}

}  // extern "C"

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi_verify)
#endif
