/*
 * kzg_bn254_mi355x.h — C-ABI of the MI355X-native KZG-BN254 prover hot path.
 *
 * Drop-in boundary for Layr-Labs/rust-kzg-bn254: the reference has no FFI seam of its own; its hot
 * path is five calls into arkworks 0.5.  Each entry point below names the
 * reference interface it replaces (file:line under /root/reference).  INTEGRATION.md shows the Rust
 * `extern "C"` binding a maintainer would add.
 *
 * Wire format (zero-copy from Rust):
 *   Fr / Fq      4 x u64 little-endian limbs, Montgomery form a * 2^256 mod m, canonical (< m) —
 *                arkworks' in-memory `Fp256<MontBackend<_, 4>>` (`fr.0.0`, cf. primitives/src/helpers.rs:158)
 *   G1 affine    8 x u64 = x[4] || y[4]; the identity is all-zero (the coordinates arkworks'
 *                `G1Affine::identity()` carries) and is also reported through `out_is_infinity`
 *   G1 partial   16 x u64 = X || Y || ZZ || ZZZ (extended Jacobian, x = X/ZZ, y = Y/ZZZ; identity: ZZ = 0)
 *
 * All pointers are caller-owned; the library never frees caller memory.  Functions return a
 * kzg_status (0 = OK, < 0 = error mirroring a `KzgError` variant, primitives/src/errors.rs:32-86).
 * A context is bound to one GPU; calls on one context are serialised internally, different
 * contexts may be used concurrently from different threads.  There is NO CPU fallback: without a
 * usable HIP device kzg_ctx_create fails with KZG_ERR_NO_DEVICE.
 *
 * ENVIRONMENT.  The library reads eleven variables and no others (csrc/engine.h `kzg::Opts`):
 *   KZG_NO_PRECOMPUTE=1, KZG_NO_NAF=1     SRS uploads without any tables / without the per-bit tables (read at every upload)
 *   KZG_HOST_THREADS_MAX, KZG_HOST_THREADS cap of (default min(48, hardware threads, the cgroup's CPU quota)) / exact width of the host pool
 *   KZG_VB_GROUP_BYTES, KZG_VB_CHUNK_BYTES, KZG_VB_TRACE   batch verification: bytes per GPU round / per upload chunk; phase times on stderr
 *                                         (KZG_VB_TRACE also prints the phases of kzg_verify_multiproof_batch, which then synchronises between them)
 *   KZG_ROCTX=1                           roctx ranges around the host phases (rocprofv3 --marker-trace)
 *   KZG_NTT_TILE_LOG=10 / 11              one tile size of the Fr NTT at every transform size
 *   KZG_EXCHANGE_TIMEOUT_S, KZG_RCCL_LIB  the _rccl entries: seconds to wait for a collective (60); the RCCL to dlopen
 * Per-context settings are calls (kzg_ctx_set_msm_window, kzg_ctx_set_reduction_lanes, kzg_ctx_set_transcript_device, kzg_ctx_set_locate_pairings, kzg_ctx_set_encode_group_bytes, kzg_ctx_set_recover_group_bytes).  Entry points marked MEASUREMENT ONLY below
 * (kzg_ctx_set_profiling, kzg_ctx_get_msm_profile*, kzg_ctx_measure_valu_rates) exist for bench.py's roofline figures; a host binding can leave them out.
 */
#ifndef KZG_BN254_MI355X_H
#define KZG_BN254_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kzg_ctx kzg_ctx;
typedef struct kzg_srs kzg_srs;

typedef enum {
    KZG_OK = 0,
    KZG_ERR_INVALID_ARG = -1,            /* null pointer / bad size */
    KZG_ERR_NO_DEVICE = -2,              /* no HIP device: the product never falls back to the CPU */
    KZG_ERR_DEVICE = -3,                 /* HIP runtime error, text in kzg_ctx_last_error */
    KZG_ERR_MSM_LENGTH_MISMATCH = -4,    /* arkworks msm Err(min_len) -> KzgError::MsmError / CommitError (helpers.rs:332, kzg.rs:102,123) */
    KZG_ERR_SRS_CAPACITY_EXCEEDED = -5,  /* KzgError::SrsCapacityExceeded (kzg.rs:89-94) */
    KZG_ERR_POLY_LENGTH = -6,            /* SerializationError("polynomial length is not correct") (kzg.rs:112-116) */
    KZG_ERR_NOT_POWER_OF_TWO = -7,       /* FFTError("length provided is not a power of 2") (kzg.rs:265-269) */
    KZG_ERR_DOMAIN = -8,                 /* domain construction failed: n > 2^28 (polynomial.rs:132-134, kzg.rs:276-278) */
    KZG_ERR_ROOTS_LENGTH = -9,           /* GenericError("inconsistent length between blob and root of unities") (kzg.rs:135-139,222-226) */
    KZG_ERR_INVALID_INPUT_LENGTH = -10,  /* KzgError::InvalidInputLength (helpers.rs:485-487) */
    KZG_ERR_TOO_LARGE = -11,             /* GenericError("Input size exceeds maximum polynomial size") (polynomial.rs:42-46) */
    KZG_ERR_ROOT_NOT_FOUND = -12,        /* GenericError("Root of unity not found") (kzg.rs:199-201) */
    KZG_ERR_ZERO_LENGTH = -13,           /* GenericError("Length of data after padding is 0") (helpers.rs:554-558) */
    KZG_ERR_SRS_LENGTH = -14,            /* GenericError("the length of data after padding is not valid with respect to the SRS") (helpers.rs:560-566) */
    KZG_ERR_DESERIALIZE = -15,           /* DeserializationError("point at infinity not coded properly for g1") (helpers.rs:191-195) */
    KZG_ERR_NOT_ON_CURVE = -16,          /* NotOnCurveError("compressed g1 point not on curve: ..") (helpers.rs:203-208) */
    KZG_ERR_G1_NOT_ON_CURVE = -17,       /* NotOnCurveError("G1 point not on curve") (helpers.rs:694-699, validate_g1_point) */
    KZG_ERR_G2_TAU_NOT_ON_CURVE = -18,   /* NotOnCurveError("Invalid trusted setup: G2_TAU not on curve") (verify.rs:29-33, batch.rs:214-216) */
    KZG_ERR_TAU_EQUALS_Z = -19,          /* GenericError("Evaluation point equals trusted setup secret") (verify.rs:56-60) */
    /* multi-rank calls only (no counterpart in the single-process reference): */
    KZG_ERR_PEER = -20,                  /* another rank of the communicator failed in this collective call (it returns its own error) */
    KZG_ERR_EXCHANGE_TIMEOUT = -21,      /* the all-gather did not complete within KZG_EXCHANGE_TIMEOUT_S (default 60): a peer is gone */
    KZG_ERR_IO = -22                     /* kzg_srs_save_packed / kzg_srs_load_packed: the file could not be opened, read or written */
} kzg_status;

/* The reference's error string for a status (Appendix B of SURVEY.md). */
const char* kzg_status_message(int32_t status);

/* ---- context -------------------------------------------------------------------------------- */
int32_t kzg_device_count(void);
int32_t kzg_ctx_create(int32_t device_id, kzg_ctx** out);
void    kzg_ctx_destroy(kzg_ctx* ctx);
const char* kzg_ctx_last_error(const kzg_ctx* ctx);
/* Tunables (0 = automatic): MSM window bits c in [2,16]; accumulate segment length.  A non-zero c also forces the
 * generic (no precomputed tables) mode for SRS-based calls. */
int32_t kzg_ctx_set_msm_window(kzg_ctx* ctx, int32_t c_bits, int32_t segment_len);
/* Lanes per point of the table-mode bucket-reduction kernels: 0 = automatic (lane quads for an MSM that runs alone, lane pairs
 * beside another MSM in flight), 2 = always pairs, 4 = always quads.  Results are identical; a test / measurement hook. */
int32_t kzg_ctx_set_reduction_lanes(kzg_ctx* ctx, int32_t lanes);
/* Where kzg_verify_multiproof_batch hashes the item digests of the weights it derives: 0 = automatic (on the device inside the envelope
 * measured to win -- at least 4 096 items of at most 64 values and 2 MiB of values: profiles/fs_device.md --, on the host pool
 * otherwise), 1 = always on the host, 2 = always on the device.
 * Results are identical; a test / measurement hook.  Another mode -> KZG_ERR_INVALID_ARG. */
int32_t kzg_ctx_set_transcript_device(kzg_ctx* ctx, int32_t mode);
/* SHA-256 of `count` messages of row_len bytes each (msgs: count x row_len bytes, message i at msgs + i * row_len), one lane per message
 * on the device (csrc/dev_sha256.h, csrc/fsdevice.hip): out_digests = count x 32 bytes.  Host buffers, synchronous.  count = 0 writes
 * nothing; row_len = 0 hashes count empty messages.  A null pointer (msgs may be NULL when row_len = 0) -> KZG_ERR_INVALID_ARG;
 * count > 2^28 or count * row_len > 2^31 -> KZG_ERR_TOO_LARGE. */
int32_t kzg_sha256_rows(kzg_ctx* ctx, const uint8_t* msgs, size_t row_len, size_t count, uint8_t* out_digests);
/* MEASUREMENT ONLY (bench.py's roofline): when enabled, every MSM launch is bracketed phase by phase with HIP events on the
 * context's launch stream.  phase_ms_out[0..7] = accumulated milliseconds of: digits, bucket scan, scatter,
 * segment map, bucket ACCUMULATE (the dominant kernel), bucket finalise, window reduction, whole device span;
 * *launches / *pairs = launches and (scalar, point) pairs covered.  Enabling resets the counters. */
int32_t kzg_ctx_set_profiling(kzg_ctx* ctx, int32_t enable);
int32_t kzg_ctx_get_msm_profile(kzg_ctx* ctx, double phase_ms_out[8], uint64_t* launches, uint64_t* pairs);
/* *entries = sorted entries (= mixed additions of the accumulate kernel) of the launches profiled since kzg_ctx_set_profiling(ctx, 1):
 * windows x pairs with the fixed-window tables, data dependent (~254 / (w + 1) + 1/2 per scalar) in the NAF mode of the per-bit tables. */
int32_t kzg_ctx_get_msm_profile_entries(kzg_ctx* ctx, uint64_t* entries);
/* MEASUREMENT ONLY: issue rate of the instruction classes the MSM accumulate kernel consists of, on this device, with
 * `waves_per_simd` waves per SIMD (the kernel runs 3): out_ns[0..5] = nanoseconds per wave-instruction per SIMD of
 * v_mad_i64_i32, v_mul_lo_u32, v_ashrrev_i64, v_and_b32, v_sub_u32 (the plain 32-bit class), s_nop.  ~60 ms of GPU time. */
int32_t kzg_ctx_measure_valu_rates(kzg_ctx* ctx, int32_t waves_per_simd, double out_ns[6]);

/* ---- SRS: device-resident monomial G1 powers -------------------------------------------------- */
/* Replaces holding `SRS.g1: Cow<[G1Affine]>` (prover/src/srs.rs:11-21) on the host and copying
 * `srs.g1[..n].to_vec()` on every commit (kzg.rs:119).  n points, 8 u64 each.  Uploaded once; for
 * 128 <= n (and table size <= 48 GiB) the upload also precomputes the window tables 2^(c w) * P_i
 * (ceil(255 / c) x 64 B per point, c = clamp(floor(log2 n) - 4, 7, 16); KZG_NO_PRECOMPUTE=1 disables). */
int32_t kzg_srs_upload(kzg_ctx* ctx, const uint64_t* g1_xy_mont, size_t n_points, kzg_srs** out);
/* SRS::new's point decoding on the GPU (prover/src/srs.rs:35-49, :51-68 -> helpers.rs:175-226 read_g1_point_from_bytes_be):
 * `bytes` = the first n_points x 32 bytes of a gnark-format compressed G1 file (big-endian x, flags in the top two bits of
 * byte 0).  All points are decompressed in one kernel (one 254-bit exponentiation per point) and the SRS is made resident
 * like kzg_srs_upload.  A malformed point -> KZG_ERR_DESERIALIZE / KZG_ERR_NOT_ON_CURVE with *bad_index = its position
 * (the reference's loader panics there, srs.rs:60-63). */
int32_t kzg_srs_load_compressed_be(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_srs** out, uint64_t* bad_index);
/* Test / bench utility (no counterpart in the reference, which loads ceremony files): synthetic SRS with a
 * KNOWN tau, P_i = tau^(first_power + i) * G1, generated on the device (a shard of the powers when
 * first_power > 0); and read-back of a resident SRS in wire format. */
int32_t kzg_srs_generate(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n_points, kzg_srs** out);
int32_t kzg_srs_download(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, size_t n, uint64_t* out_xy_mont);
/* A loaded SRS written once in the library's own packed form and read back WITHOUT decoding (the reference decodes the ceremony
 * file at every SRS::new, prover/src/srs.rs:35-188 -- one field exponentiation per point; its README quotes "a few minutes" for the mainnet file):
 * "KZGSRS1\0" | u64 n | u64 0 | SHA-256 of the payload | n x 64 B points exactly as kzg_srs_upload takes them.  Loading verifies the digest
 * (KZG_ERR_DESERIALIZE: wrong magic, truncated, trailing bytes, digest mismatch) and, on the device, that every point is on the curve or the
 * identity (KZG_ERR_NOT_ON_CURVE), then builds the tables like kzg_srs_upload.  points_to_load = 0: all of them; more than the file holds ->
 * KZG_ERR_SRS_LENGTH; a file that cannot be opened / written -> KZG_ERR_IO. */
int32_t kzg_srs_save_packed(kzg_ctx* ctx, const kzg_srs* srs, const char* path);
int32_t kzg_srs_load_packed(kzg_ctx* ctx, const char* path, size_t points_to_load, kzg_srs** out);
void    kzg_srs_free(kzg_srs* srs);
size_t  kzg_srs_len(const kzg_srs* srs);
/* The same loader for the "native" format of SRS::parallel_read_g1_points_native(.., is_native = true) (prover/src/srs.rs:205-251 ->
 * primitives/src/traits.rs:34-36: G1Affine::deserialize_compressed of ark-serialize 0.5): x as 32 little-endian bytes, flags in the top
 * two bits of the LAST byte (0x80 = the larger y, 0x40 = infinity; both set, or x >= p -> KZG_ERR_DESERIALIZE).  RESTATED from
 * ark-serialize, not pinned by a reference vector: the reference tree holds no file in this format and calls the function nowhere. */
int32_t kzg_srs_load_compressed_ark_le(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_srs** out, uint64_t* bad_index);
/* 1 when the SRS carries its per-bit tables Bit_p[i] = 2^p P_i (the NAF mode of MSMs of >= 2^14 pairs and the batched launches need
 * them; absent with KZG_NO_NAF=1, above 2^22 points, or when HBM is short).  build != 0: try to build them first (once, on the SRS's
 * own context).
 *
 * THREADS.  An SRS handle may be used from any number of host threads and by every context of its GPU at once, as the reference shares
 * one `SRS` across threads (prover/tests/kzg_test.rs:9-17, primitives/tests/blob_test.rs:83-94).  Tables that are built after upload
 * -- these per-bit tables on the first batched call of a small SRS, the x3 / x5 / x7 tables of kzg_g1_ifft(64..2048) (<= 100 MB, built on the first such call), the bases attached by
 * kzg_srs_cache_lagrange -- are built under a lock of the SRS and published only when complete; calls on ONE context are serialised by
 * the context's own lock, so N threads sharing a context see N serial calls; threads that need to overlap use one context each
 * (contexts of one GPU share the SRS).  kzg_srs_free / kzg_srs_drop_lagrange must not race with calls that use the handle.
 * tests/test_gpu_concurrency.py exercises exactly this contract. */
int32_t kzg_srs_has_bit_tables(kzg_srs* srs, int32_t build);

/* ---- arkworks boundary 1: <G1Projective as VariableBaseMSM>::msm(bases, scalars).into_affine() -- */
/* Call sites: prover/src/kzg.rs:100, :121; primitives/src/helpers.rs:332 (g1_lincomb).
 * n_bases != n_scalars -> KZG_ERR_MSM_LENGTH_MISMATCH (arkworks returns Err(min_len)). */
int32_t kzg_msm_g1(kzg_ctx* ctx, const uint64_t* bases_xy_mont, size_t n_bases,
                   const uint64_t* scalars_mont, size_t n_scalars,
                   uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
/* `batch` independent MSMs of n pairs each in one kernel sequence: bases = batch x n points, scalars = batch x n
 * elements (MSM b uses the b-th block of each), out = batch x 8 u64 (+ batch infinity flags).  This is the shape of
 * verifier/src/batch.rs:228,245,246 (three g1_lincomb calls of equal length); results equal `batch` kzg_msm_g1 calls. */
int32_t kzg_msm_g1_batch(kzg_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars_mont, size_t n, size_t batch,
                         uint64_t* out_xy_mont, uint8_t* out_is_infinity);
/* Same with bases = srs[offset .. offset + n) already resident (commit path). */
int32_t kzg_msm_g1_srs(kzg_ctx* ctx, const kzg_srs* srs, size_t offset,
                       const uint64_t* scalars_mont, size_t n,
                       uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
/* Scalars already in device memory (d_scalars_mont: device pointer to n x 4 u64). */
int32_t kzg_msm_g1_srs_device(kzg_ctx* ctx, const kzg_srs* srs, size_t offset,
                              const void* d_scalars_mont, size_t n,
                              uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
/* Multi-GPU sharding: partial sum of one shard, not converted to affine (16 u64 XYZZ). */
int32_t kzg_msm_g1_srs_partial_device(kzg_ctx* ctx, const kzg_srs* srs, size_t offset,
                                      const void* d_scalars_mont, size_t n, uint64_t out_xyzz_mont[16]);
int32_t kzg_msm_g1_srs_partial(kzg_ctx* ctx, const kzg_srs* srs, size_t offset,
                               const uint64_t* scalars_mont, size_t n, uint64_t out_xyzz_mont[16]);
#ifndef KZG_NUM_SLOTS
#define KZG_NUM_SLOTS 4
#endif
/* Asynchronous form for streams of commitments (software pipelining): `begin` enqueues the whole kernel sequence of one
 * MSM over srs[offset .. offset + n) on the stream of `slot` (0 .. KZG_NUM_SLOTS-1; each slot has its own stream and workspace) and
 * returns without waiting; `end` waits for that slot, runs the O(1) host epilogue and writes the affine point
 * (out_xy_mont / out_is_infinity) and/or the unconverted partial sum (out_xyzz_mont, 16 u64); either may be NULL.
 * With begin(k+1) issued before end(k), the sort / bucket-reduction phases of one MSM run beside the accumulation of the
 * other and the host epilogue leaves the critical path.  d_scalars_mont must be complete before `begin` and stay
 * untouched until `end`.  1 <= n <= 2^26 (at most 64 launches: an SRS of more than 2^20 points is served in launches of 2^20 pairs;
 * the synchronous calls have no cap; the asynchronous commit_eval_form / commit_blob / compute_proof forms below stop at 2^24);
 * a slot that is still in flight (or, for `end`, idle) -> KZG_ERR_INVALID_ARG.
 * The synchronous MSM / commit / proof calls use slot 0's workspace: while slot 0 is in flight they return
 * KZG_ERR_INVALID_ARG (text in kzg_ctx_last_error); the other slots may be in flight beside them.  Two slots hide the latency-bound
 * phases of a 2^20-pair MSM; shard-sized MSMs (2^17 .. 2^18 pairs per GPU) keep gaining up to four. */
int32_t kzg_msm_g1_srs_device_begin(kzg_ctx* ctx, const kzg_srs* srs, size_t offset,
                                    const void* d_scalars_mont, size_t n, int32_t slot);
/* Same with the scalars in host memory (n x 4 u64): the H2D copy is issued on the slot's stream into the slot's staging
 * buffer, so with two slots alternating it runs beside the other slot's kernels.  The host buffer may be reused as soon as
 * `begin` returns only if it is pageable memory (the runtime stages it); a pinned buffer must stay valid until `end`. */
int32_t kzg_msm_g1_srs_begin(kzg_ctx* ctx, const kzg_srs* srs, size_t offset,
                             const uint64_t* scalars_mont, size_t n, int32_t slot);
int32_t kzg_msm_g1_srs_end(kzg_ctx* ctx, int32_t slot, uint64_t* out_xy_mont, uint8_t* out_is_infinity,
                           uint64_t* out_xyzz_mont);
/* Fold `count` gathered partial sums (count x 16 u64) and convert to affine.  Host-only, O(count). */
int32_t kzg_g1_fold_partials(const uint64_t* partials_xyzz_mont, size_t count,
                             uint64_t out_xy_mont[8], uint8_t* out_is_infinity);

/* ---- arkworks boundary 2: GeneralEvaluationDomain::<Fr>::new(n).{fft,ifft}(&[Fr]) --------------- */
/* Call sites: primitives/src/polynomial.rs:131-135 (ifft), :242-246 (fft).  Natural order in and out,
 * omega = 5^((r-1)/n); the inverse transform includes the n^-1 scaling.  In place.
 * n not a power of two -> KZG_ERR_NOT_POWER_OF_TWO; n > 2^28 -> KZG_ERR_DOMAIN. */
int32_t kzg_fr_ntt(kzg_ctx* ctx, uint64_t* data_mont, size_t n, int32_t inverse);
int32_t kzg_fr_ntt_device(kzg_ctx* ctx, void* d_data_mont, size_t n, int32_t inverse);

/* ---- KZG surface (prover/src/kzg.rs) ----------------------------------------------------------- */
/* KZG::commit_coeff_form (kzg.rs:107-125): n > srs len -> KZG_ERR_POLY_LENGTH. */
int32_t kzg_commit_coeff_form(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* coeffs_mont, size_t n,
                              uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
/* Batched forms (no counterpart in the reference, which commits one polynomial per call): `count` polynomials of n coefficients
 * (evaluations) each, one after the other in memory, against the first n points of ONE SRS -> count commitments, out_xy_mont = count x 8
 * words, out_is_infinity = count bytes (may be NULL).  Same values and errors as count calls of kzg_commit_coeff_form /
 * kzg_commit_eval_form; ONE kernel sequence per 1 024 polynomials (width-8 NAF digits over the SRS's per-bit tables, 64 buckets per
 * polynomial): a few microseconds per commitment of 512..2048 coefficients instead of 0.14-0.2 ms.  The SRS handle is not const:
 * an SRS of fewer than 2^15 points gets its per-bit tables (16 KiB per point) on the first batched call, and the eval form keeps
 * the Lagrange basis of n points with the SRS (kzg_srs_cache_lagrange).  _device: the scalars are already in device memory. */
int32_t kzg_commit_coeff_form_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* coeffs_mont, size_t n, size_t count,
                                    uint64_t* out_xy_mont, uint8_t* out_is_infinity);
int32_t kzg_commit_coeff_form_batch_device(kzg_ctx* ctx, kzg_srs* srs, const void* d_coeffs_mont, size_t n, size_t count,
                                           uint64_t* out_xy_mont, uint8_t* out_is_infinity);
int32_t kzg_commit_eval_form_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* evals_mont, size_t n, size_t count,
                                   uint64_t* out_xy_mont, uint8_t* out_is_infinity);
int32_t kzg_commit_eval_form_batch_device(kzg_ctx* ctx, kzg_srs* srs, const void* d_evals_mont, size_t n, size_t count,
                                          uint64_t* out_xy_mont, uint8_t* out_is_infinity);
/* ONE batched launch, asynchronous (the building block of the calls above, for streams of resident scalar sets -- e.g. the ranks of a
 * sharded commitment, which group several steps into one launch): `count` scalar sets of n scalars each, in SEPARATE device buffers,
 * against srs[offset .. offset + n) on `slot`; count <= min(16, kzg_msm_batch_capacity(n)).  _end_batch waits and returns count affine
 * points (count x 8 words) and / or count XYZZ partials (count x 16 words), in order. */
size_t kzg_msm_batch_capacity(size_t n);
int32_t kzg_msm_g1_srs_device_begin_batch(kzg_ctx* ctx, kzg_srs* srs, size_t offset, const void* const* d_scalars_mont, size_t n, size_t count, int32_t slot);
int32_t kzg_msm_g1_srs_end_batch(kzg_ctx* ctx, int32_t slot, size_t count, uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint64_t* out_xyzz_mont);
/* KZG::commit_eval_form (kzg.rs:84-104): n > srs len -> KZG_ERR_SRS_CAPACITY_EXCEEDED; n not a power of
 * two -> KZG_ERR_NOT_POWER_OF_TWO.  Computed as MSM(srs, IFFT(evals)), identical to the reference's
 * MSM(g1_ifft(srs), evals) (prover/src/lib.rs:43-47; prover/tests/kzg_test.rs:57-89). */
int32_t kzg_commit_eval_form(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n,
                             uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
/* helpers::to_fr_array + PolynomialEvalForm::new padding (helpers.rs:40-57, polynomial.rs:41-57): each 32-byte big-endian
 * chunk of the (already padded) blob mod r, last chunk right-padded with zeros, zero-extended to the next power of two;
 * *n_out = that length; out needs cap >= *n_out elements (call with out = NULL to query). */
int32_t kzg_blob_to_fr(kzg_ctx* ctx, const uint8_t* blob_bytes, size_t len, uint64_t* out_mont, size_t cap, size_t* n_out);
/* KZG::commit_blob (kzg.rs:182-185) = Blob::to_polynomial_eval_form + commit_eval_form, bytes in, point out. */
int32_t kzg_commit_blob(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len,
                        uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
/* Asynchronous forms of the two calls above for streams of blobs: the whole chain (H2D copy, bytes -> Fr, IFFT, MSM) is
 * enqueued on the stream of `slot`; collect the commitment with kzg_msm_g1_srs_end(ctx, slot, ...).  Host input
 * buffers follow the rule of kzg_msm_g1_srs_begin.  Same error codes as the synchronous calls; n (resp. the padded blob
 * length) <= 2^24. */
int32_t kzg_commit_eval_form_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n, int32_t slot);
int32_t kzg_commit_blob_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, int32_t slot);
/* KZG::g1_ifft (kzg.rs:263-285): Lagrange-basis SRS L_i = n^-1 sum_j w^(-ij) P_j of the first n SRS points, natural
 * order, n x 8 u64 written to out.  n not a power of two -> KZG_ERR_NOT_POWER_OF_TWO ("length provided is not a
 * power of 2"); n > 2^28 -> KZG_ERR_DOMAIN.  Not used by the commit / proof path of this library. */
int32_t kzg_g1_ifft(kzg_ctx* ctx, const kzg_srs* srs, size_t n, uint64_t* out_xy_mont);
/* The same Lagrange basis kept ON THE DEVICE.  The reference recomputes g1_ifft inside every commit_eval_form
 * (prover/src/kzg.rs:96-98); here it is computed once per (SRS, n):
 *   kzg_srs_cache_lagrange  builds it (with its MSM window tables) and attaches it to `srs`; from then on kzg_commit_eval_form of
 *                           exactly n evaluations is ONE MSM over it (the reference's literal form, kzg.rs:98-100) instead of
 *                           IFFT + MSM over the monomial basis -- the same point either way;
 *   kzg_srs_lagrange        returns it as an SRS handle of its own (free with kzg_srs_free): kzg_msm_g1_srs over it with the
 *                           evaluations as scalars is commit_eval_form;
 *   kzg_srs_drop_lagrange   releases what kzg_srs_cache_lagrange attached.
 * Errors as kzg_g1_ifft. */
int32_t kzg_srs_cache_lagrange(kzg_ctx* ctx, kzg_srs* srs, size_t n);
int32_t kzg_srs_lagrange(kzg_ctx* ctx, const kzg_srs* srs, size_t n, kzg_srs** out);
int32_t kzg_srs_drop_lagrange(kzg_ctx* ctx, kzg_srs* srs);
/* Proofs for EVERY coset of the domain in one call (Feist-Khovratovich "FK20", eprint 2023/033): the generalisation of
 * KZG::compute_proof_with_known_z_fr_index (prover/src/kzg.rs:187-234), which opens one point per call, to all of them in O(n log n).
 * poly: n Fr elements (n x 4 u64), evaluations on the domain {w^i} (eval_form = 1; inverse-NTT'd on the device) or coefficients
 * (eval_form = 0); w the library's primitive n-th root (kzg_calculate_roots_of_unity).  chunk_len = l, a power of two with
 * 1 <= l <= n / 2, m = n / l.  Chunk k < m is the coset {w^(k + j m) : j < l}, i.e. evaluation indices k, k + m, k + 2m, ...; its
 * proof is [q_k(tau)]_1 with q_k = f / (X^l - w^(k l)).  For l = 1 proof k is exactly kzg_compute_proof's proof at z = w^k.
 * out_xy: m x 8 u64 affine wire points (the identity as zeros), out_is_infinity: m flags.
 * The 2n points FFT_2m(S^(b)) of FK20 depend on (srs, n, l) only: the first call builds them and keeps them on `srs`
 * (kzg_srs_cache_multiproof builds them up front; kzg_srs_drop_multiproof and kzg_srs_free release them).
 * Errors: a null pointer, srs of another context, a Lagrange-basis handle, n = 1, l not a power of two or l > n / 2 ->
 * KZG_ERR_INVALID_ARG; n = 0 or not a power of two -> KZG_ERR_NOT_POWER_OF_TWO; n > 2^24 -> KZG_ERR_DOMAIN; n > kzg_srs_len(srs) ->
 * KZG_ERR_SRS_CAPACITY_EXCEEDED; a failed allocation -> KZG_ERR_DEVICE (kzg_ctx_last_error has the text). */
int32_t kzg_compute_multiproofs(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, size_t n, int32_t eval_form,
                                size_t chunk_len, uint64_t* out_xy_mont, uint8_t* out_is_infinity);
int32_t kzg_srs_cache_multiproof(kzg_ctx* ctx, kzg_srs* srs, size_t n, size_t chunk_len);
int32_t kzg_srs_drop_multiproof(kzg_ctx* ctx, kzg_srs* srs);
/* The encoder of a data-availability scheme: a blob of d = poly_len coefficients, evaluated on the domain of n = r d points (rate 1/r)
 * and handed out as the m = n / l cosets of l = chunk_len values, each with its proof -- kzg_compute_multiproofs aware of the degree
 * bound deg f < d <= n.  The conventions are kzg_compute_multiproofs': w the library's primitive n-th root, coset k < m is
 * {w^(k + j m) : j < l}, its proof [f / (X^l - w^(k l))](tau) G1.  Every quotient has degree < d - l, so the SRS needs d points, not n,
 * and the FK20 table is the (d, l) entry that kzg_srs_cache_multiproof(srs, d, l) builds (2d points); only the last transform, m points
 * of which m / r are not the identity, sees n.  With n = poly_len the proofs are those of kzg_compute_multiproofs.
 * poly: d Fr elements, coefficients (eval_form = 0) or evaluations on the d-point domain {(w^r)^i} (eval_form = 1; inverse-NTT'd on
 * the device).  out_ys: m x l x 4 u64 canonical wire words, ys[k][j] = f(w^(k + j m)), the rows kzg_verify_multiproof* and
 * kzg_recover_from_cosets take.  out_proofs_xy: m x 8 u64 affine wire points (the identity as zeros), out_is_infinity: m flags, required
 * when proofs are asked for.  Either output may be NULL (it is then not computed), not both.
 * Errors, checked on the host before any kernel runs, in this order:
 *   1. a null ctx, srs or poly; both outputs NULL; proofs without flags -> KZG_ERR_INVALID_ARG;
 *   2. srs of another context, or a Lagrange-basis handle -> KZG_ERR_INVALID_ARG;
 *   3. poly_len or n zero or not a power of two -> KZG_ERR_NOT_POWER_OF_TWO;
 *   4. n > 2^24 -> KZG_ERR_DOMAIN;
 *   5. poly_len > n, poly_len = 1, chunk_len not a power of two or > poly_len / 2 -> KZG_ERR_INVALID_ARG;
 *   6. poly_len > kzg_srs_len(srs) -> KZG_ERR_SRS_CAPACITY_EXCEEDED.
 * A failed allocation -> KZG_ERR_DEVICE (kzg_ctx_last_error has the text).  After any error the context stays usable. */
int32_t kzg_encode_cosets(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, size_t poly_len /* d */, int32_t eval_form,
                          size_t n, size_t chunk_len, uint64_t* out_ys_mont /* m x chunk_len x 4, may be NULL */,
                          uint64_t* out_proofs_xy_mont /* m x 8, may be NULL */, uint8_t* out_is_infinity /* m */);
/* kzg_encode_cosets for `count` blobs of one shape (d, n, l, eval_form) in one call.  polys: count x d Fr elements, blob b at
 * polys + b d 4; row b of every output (out_ys: count x m x l x 4, out_proofs_xy: count x m x 8, out_is_infinity: count x m) is
 * bit-identical to kzg_encode_cosets on blob b.  The FK20 table is the same (d, l) entry, built once.  The call works through the
 * blobs in GROUPS whose device workspace fits a byte budget (4 GiB unless kzg_ctx_set_encode_group_bytes says otherwise; a group is
 * never smaller than one blob, count has no cap): inside a group every stage is one launch for all its blobs, with the stage plan
 * of the two G1 transforms chosen for the group, and there is one upload and one download per output array.  A shape whose
 * single-blob stages already fill the device (every scalar-multiplication stage has >= 65 536 lanes) runs as groups of one, through
 * the launches of kzg_encode_cosets.
 * Errors, checked on the host before any kernel runs, in this order:
 *   1. a null ctx, srs or polys; both outputs NULL; proofs without flags; count = 0 -> KZG_ERR_INVALID_ARG;
 *   2. srs of another context, or a Lagrange-basis handle -> KZG_ERR_INVALID_ARG;
 *   3. poly_len or n zero or not a power of two -> KZG_ERR_NOT_POWER_OF_TWO;
 *   4. n > 2^24 -> KZG_ERR_DOMAIN;
 *   5. poly_len > n, poly_len = 1, chunk_len not a power of two or > poly_len / 2 -> KZG_ERR_INVALID_ARG;
 *   6. poly_len > kzg_srs_len(srs) -> KZG_ERR_SRS_CAPACITY_EXCEEDED;
 *   7. a count whose output sizes (count x n x 64 bytes) overflow size_t -> KZG_ERR_INVALID_ARG.
 * A failed allocation -> KZG_ERR_DEVICE (kzg_ctx_last_error has the text).  After any error the context stays usable. */
int32_t kzg_encode_cosets_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont /* count x d x 4 */, size_t count,
                                size_t poly_len /* d */, int32_t eval_form, size_t n, size_t chunk_len,
                                uint64_t* out_ys_mont /* count x m x l x 4, may be NULL */,
                                uint64_t* out_proofs_xy_mont /* count x m x 8, may be NULL */, uint8_t* out_is_infinity /* count x m */);
/* The workspace budget of a group of kzg_encode_cosets_batch on this context, in bytes; 0 = the default (4 GiB). */
int32_t kzg_ctx_set_encode_group_bytes(kzg_ctx* ctx, size_t bytes);
/* What kzg_encode_cosets_batch would do with these arguments: a pure query (no context, no device).  values / proofs: which outputs
 * are asked for; group_bytes: the budget, 0 = the default.  Errors: out NULL or neither output -> KZG_ERR_INVALID_ARG, then rows 3, 4,
 * 5 and 7 of the table above. */
enum { KZG_ENCODE_FORM_NONE = 0, KZG_ENCODE_FORM_COPY = 1, KZG_ENCODE_FORM_DIRECT = 2, KZG_ENCODE_FORM_RADIX2 = 3 };
enum { KZG_ENCODE_LOAD_IN_PLACE = 0,   /* the first stage reads the input where it is */
       KZG_ENCODE_LOAD_COPY = 1,       /* a copy of the strided slice */
       KZG_ENCODE_LOAD_BITREV = 2,     /* a bit-reversed copy (radix-2) */
       KZG_ENCODE_LOAD_PAD = 3,        /* the padding copy (direct stages, r >= 2) */
       KZG_ENCODE_LOAD_SPREAD = 4 };   /* the spread load (radix-2, r >= 2) */
typedef struct kzg_encode_transform_info {
    int32_t form;      /* KZG_ENCODE_FORM_*; NONE: no proofs asked for */
    int32_t pairs;     /* 1: the stages run on lane pairs, 0: on lanes */
    int32_t stages;    /* stages that multiply points (each one scalar multiplication deep) */
    int32_t load;      /* KZG_ENCODE_LOAD_* */
} kzg_encode_transform_info;
typedef struct kzg_encode_batch_info {
    uint64_t blobs_per_group;            /* the last group of a call may hold fewer */
    uint64_t groups;
    uint64_t group_bytes;                /* device workspace of one full group */
    int32_t batched;                     /* 0: the groups-of-one rule applies to this shape */
    int32_t reserved;
    kzg_encode_transform_info inverse;   /* the inverse G1 FFT of 2d / l points, as planned for a full group */
    kzg_encode_transform_info forward;   /* the zero-padded forward G1 FFT of n / l points */
} kzg_encode_batch_info;
int32_t kzg_encode_cosets_batch_info(size_t poly_len /* d */, size_t n, size_t chunk_len, size_t count, int32_t values, int32_t proofs,
                                     size_t group_bytes, kzg_encode_batch_info* out);
/* The values and the proofs of SELECTED cosets of polynomials the caller holds, without computing every proof: what a node answers a
 * sampling request with, what a disperser re-sends, what a retriever re-seeds after kzg_recover_from_cosets.  The conventions are
 * kzg_encode_cosets': polys holds `count` polynomials of d = poly_len elements each (coefficients, or with eval_form = 1 evaluations on
 * the d-point domain; each REFERENCED polynomial is inverse-NTT'd once on the device), n = r d, l = chunk_len, m = n / l.
 * n_items (polynomial, coset) pairs: item i is coset coset_indices[i] < m of polynomial poly_indices[i] < count (poly_indices NULL: every
 * item is of polynomial 0).  Row i of out_ys (n_items x l x 4) and out_proofs_xy (n_items x 8) / out_is_infinity (n_items) is bit for bit
 * row coset_indices[i] of kzg_encode_cosets on that polynomial.  Either output may be NULL (it is then not computed), not both.
 * Per item the device divides f by X^l - w^(k l) (d field products in lanes of at most 64 dependent ones; the remainder gives the values
 * through one l-point NTT) and commits the quotient over the first d points of the SRS: k d MSM terms for k items, against the 2d
 * scalar multiplications and two G1 FFTs of the encoder -- the cheaper route for a few cosets (profiles/prove_cosets.md has the
 * crossover).  The items are worked through in GROUPS whose device workspace (per item: its d x 32-byte quotient row, the segment heads,
 * the remainder) fits the budget of kzg_ctx_set_encode_group_bytes (default 4 GiB; a group is never smaller than one item; the bits do
 * not depend on it); the proofs of a group are one batched commitment (kzg_commit_coeff_form_batch's path: the SRS gets its per-bit
 * tables on first use), of a group of one item a single MSM.  Duplicate items are allowed and give equal rows.
 * Errors, checked on the host before any kernel runs, in this order:
 *   1. a null ctx, srs, polys or coset_indices; both outputs NULL; proofs without flags; count = 0 -> KZG_ERR_INVALID_ARG;
 *   2. srs of another context, or a Lagrange-basis handle -> KZG_ERR_INVALID_ARG;
 *   3. rows 3, 4, 5 and 6 of kzg_encode_cosets' table, with its codes;
 *   4. a polynomial index >= count or a coset index >= m -> KZG_ERR_INVALID_ARG, *bad_index (may be NULL) = the smallest such item;
 *   5. sizes that overflow size_t (count x d x 32 bytes, n_items x the largest output row) -> KZG_ERR_INVALID_ARG.
 * n_items = 0 (after these checks) -> KZG_OK, nothing written, no device work.  The call is synchronous on slot 0: while a kzg_*_begin
 * is in flight there it returns KZG_ERR_INVALID_ARG (with proofs: while one is in flight on any slot, as the batched commitments use
 * them all).  A failed allocation -> KZG_ERR_DEVICE.  After any error the context stays usable. */
int32_t kzg_prove_cosets(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont /* count x d x 4 */, size_t count, size_t poly_len /* d */,
                         int32_t eval_form, size_t n, size_t chunk_len, const uint64_t* poly_indices /* n_items, may be NULL */,
                         const uint64_t* coset_indices /* n_items */, size_t n_items, uint64_t* out_ys_mont /* n_items x l x 4, may be NULL */,
                         uint64_t* out_proofs_xy_mont /* n_items x 8, may be NULL */, uint8_t* out_is_infinity /* n_items */, uint64_t* bad_index);
/* The quotient polynomials themselves: row i of out_q (n_items x d x 4 canonical wire words, the top l of each row zero) holds the
 * coefficients of f / (X^l - w^(k l)) for item i, and / or the values out_ys as above: no SRS.  Either output may be NULL, not both.
 * The errors are those of kzg_prove_cosets without the SRS (no check 2, no row 6), the largest output row being d x 32 bytes. */
int32_t kzg_coset_quotients(kzg_ctx* ctx, const uint64_t* polys_mont /* count x d x 4 */, size_t count, size_t poly_len /* d */, int32_t eval_form,
                            size_t n, size_t chunk_len, const uint64_t* poly_indices /* n_items, may be NULL */, const uint64_t* coset_indices,
                            size_t n_items, uint64_t* out_q_mont /* n_items x d x 4, may be NULL */, uint64_t* out_ys_mont, uint64_t* bad_index);
/* What kzg_prove_cosets would do with these arguments: a pure query (no context, no device).  values / proofs: which outputs are asked
 * for (proofs: the quotient rows are kept, as kzg_coset_quotients with out_q does); group_bytes: the budget, 0 = the default.  Errors: out
 * NULL, neither output or count = 0 -> KZG_ERR_INVALID_ARG, then rows 3, 4 and 5 of kzg_encode_cosets' table and check 5 above. */
typedef struct kzg_prove_cosets_info_t {    /* (_t: C has one name space for the struct and the function) */
    uint64_t items_per_group;            /* the last group of a call may hold fewer */
    uint64_t groups;
    uint64_t group_bytes;                /* device workspace of one full group */
    uint64_t item_bytes;                 /* of one item */
    uint32_t seg_len;                    /* S: the most dependent field products a lane runs in one pass */
    uint32_t segments;                   /* segments of one chain of d / l coefficients */
    uint32_t carry_levels;               /* passes of the same recurrence over the segment heads (0: a chain is one segment) */
    uint32_t launches;                   /* kernel launches of a group in front of the MSM: local and fix-up passes, the values' NTT passes */
    uint32_t msm_single;                 /* 1: a group is one item and its proof is a single MSM, 0: a batched commitment */
    uint32_t reserved;
} kzg_prove_cosets_info_t;
int32_t kzg_prove_cosets_info(size_t poly_len /* d */, size_t n, size_t chunk_len, size_t count, size_t n_items, int32_t values, int32_t proofs,
                              size_t group_bytes, kzg_prove_cosets_info_t* out);
/* KZG::compute_proof / compute_proof_impl (kzg.rs:128-178, :215-234, on-domain branch :237-260).
 * roots = KZG::expanded_roots_of_unity (n_roots entries); n != n_roots -> KZG_ERR_ROOTS_LENGTH.
 * out_y (optional, 4 u64) receives y = p(z) (helpers.rs:475-535). */
int32_t kzg_compute_proof(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n,
                          const uint64_t* roots_mont, size_t n_roots, const uint64_t z_mont[4],
                          uint64_t out_xy_mont[8], uint8_t* out_is_infinity, uint64_t* out_y_mont);
/* Asynchronous form of kzg_compute_proof for streams of proofs (same slots as kzg_msm_g1_srs_begin): upload, batch inversion,
 * y, quotient, IFFT and MSM are all enqueued on the slot's stream; `end` waits and returns the proof point and y = p(z). */
int32_t kzg_compute_proof_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n,
                                const uint64_t* roots_mont, size_t n_roots, const uint64_t z_mont[4], int32_t slot);
int32_t kzg_compute_proof_end(kzg_ctx* ctx, int32_t slot, uint64_t out_xy_mont[8], uint8_t* out_is_infinity,
                              uint64_t* out_y_mont);
/* Multi-GPU forms of the two calls above (BASELINE config 4).  srs_shard holds the SRS powers
 * [shard_lo, shard_lo + kzg_srs_len(srs_shard)); every rank passes the whole polynomial, performs the O(n) field work
 * (IFFT, quotient) redundantly and commits only its slice of the coefficients; out = the unconverted partial sum (16 u64)
 * that the ranks all-gather and fold with kzg_g1_fold_partials.  The shards must jointly cover [0, n). */
int32_t kzg_commit_eval_form_partial(kzg_ctx* ctx, const kzg_srs* srs_shard, size_t shard_lo,
                                     const uint64_t* evals_mont, size_t n, uint64_t out_xyzz_mont[16]);
int32_t kzg_compute_proof_partial(kzg_ctx* ctx, const kzg_srs* srs_shard, size_t shard_lo,
                                  const uint64_t* evals_mont, size_t n, const uint64_t* roots_mont, size_t n_roots,
                                  const uint64_t z_mont[4], uint64_t out_xyzz_mont[16], uint64_t* out_y_mont);
/* ---- BASELINE config 4 sharded by EVALUATION index over the Lagrange basis (csrc/lagrange.hip) --------------------------
 * The reference commits an evaluation-form polynomial as MSM(g1_ifft(srs), evals) (prover/src/kzg.rs:96-100) and a proof as the same MSM
 * over the evaluations of the quotient q_i = (f_i - y) / (w^i - z) (kzg.rs:151-177; the entry of a domain point z = w^m: kzg.rs:237-260).
 * Both are sums over the evaluation index, so a rank that holds the Lagrange points L_i and the evaluations f_i of a contiguous index
 * range [lo, lo + len) needs nothing else: it uploads, inverts and divides its OWN slice (4 MiB at n = 2^20 over 8 ranks) -- no replicated
 * upload, no IFFT, no whole-polynomial quotient (the kzg_*_partial forms above do all three on every rank).  Two small exchanges per proof:
 *     phase 1   S_g = sum_{i in slice} f_i w^i / (z - w^i)   ->  all-gather of G x 64 B  ->  y = (z^n - 1) / n sum_g S_g   (helpers.rs:507-532;
 *               z = w^m: y = f_m, sent by the slice that owns m, helpers.rs:497-504)
 *     phase 2   q_i on the slice, MSM over the slice          ->  all-gather of G x 256 B ->  proof = fold of the partial points (+ q_m L_m)
 * Results are the SAME field elements and the same affine point as kzg_compute_proof / kzg_commit_eval_form on one GPU.
 *
 * kzg_srs_slice            a copy of srs[lo, lo + len) as an SRS handle of its own (its own window / per-bit tables)
 * kzg_srs_lagrange_shard   KZG::g1_ifft(n) of the first n points of `srs` (kzg.rs:263-285), of which the points [lo, lo + len) are kept as a
 *                          handle of their own: this rank's shard of the Lagrange basis (one-time set-up; errors as kzg_g1_ifft).  A host that
 *                          already holds the Lagrange points uploads its slice with kzg_srs_upload instead. */
int32_t kzg_srs_slice(kzg_ctx* ctx, const kzg_srs* srs, size_t lo, size_t len, kzg_srs** out);
int32_t kzg_srs_lagrange_shard(kzg_ctx* ctx, const kzg_srs* srs, size_t n, size_t lo, size_t len, kzg_srs** out);
/* KZG::commit_eval_form (kzg.rs:84-104) of this rank's slice: sum_{i in slice} f_i L_i, unconverted (16 words, folded with
 * kzg_g1_fold_partials).  len > kzg_srs_len(lagrange_shard) -> KZG_ERR_SRS_CAPACITY_EXCEEDED. */
int32_t kzg_commit_eval_form_lagrange_partial(kzg_ctx* ctx, const kzg_srs* lagrange_shard, const uint64_t* evals_slice_mont, size_t len,
                                              uint64_t out_xyzz_mont[16]);
int32_t kzg_commit_eval_form_lagrange_partial_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, const void* d_evals_slice_mont, size_t len,
                                                     uint64_t out_xyzz_mont[16]);
/* KZG::compute_proof_impl (kzg.rs:128-178) on a slice, in four steps on `slot` (the asynchronous slots of kzg_msm_g1_srs_begin; several
 * proofs may be in flight on different slots):
 *   _begin       enqueue: upload of the slice (or, _device, the caller's resident buffer read in place: keep it untouched until _end),
 *                the inverses 1 / (w^i - z) of the slice (one inversion per 1 024 elements, side by side; they need z only and run BESIDE the upload)
 *                and S_g.  A pageable host buffer may be reused when _begin returns (the runtime has staged it); a PINNED one must stay valid and
 *                unchanged until _partial_y has returned, as for kzg_msm_g1_srs_begin.  shard_lo = index of the
 *                slice's first evaluation; shard_lo + len <= n, len <= kzg_srs_len(lagrange_shard), n a power of two <= 2^28.
 *   _partial_y   waits for phase 1: out_ypart = 8 words, S_g | f_m (f_m only from the slice that owns m when z = w^m, else zero)
 *   kzg_lagrange_fold_y        (host only) y from the G gathered 8-word parts
 *   _continue    enqueue: y goes up, q_i on the slice, the slice's MSM over the Lagrange shard
 *   _end         waits: out_part = 32 words: [0,16) XYZZ partial | [16,20) T_g = sum_{i != m} q_i w^i (z = w^m only) | [20,28) L_m, [28] = 1
 *                (the owner of m only) | zeros
 *   kzg_lagrange_fold_proof    (host only) the proof point from the G gathered 32-word parts (z = w^m: + q_m L_m, q_m = -(1/z) sum_g T_g)
 *   _abort       gives up whatever the slot has in flight (a peer failed between two phases)
 * An empty slice (len = 0) is valid in every step and contributes zeros / the identity.  A step called out of order, or on a slot that is
 * busy otherwise -> KZG_ERR_INVALID_ARG. */
#define KZG_LAGRANGE_YPART_WORDS 8
#define KZG_LAGRANGE_PART_WORDS 32
int32_t kzg_compute_proof_lagrange_begin(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const uint64_t* evals_slice_mont,
                                         size_t len, size_t n, const uint64_t z_mont[4], int32_t slot);
int32_t kzg_compute_proof_lagrange_begin_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const void* d_evals_slice_mont,
                                                size_t len, size_t n, const uint64_t z_mont[4], int32_t slot);
/* Commitment AND proof of one slice, for streams of blobs (BASELINE config 4 per rank, several blobs in flight): as _begin on `proof_slot`, and the
 * slice's commitment sum_i f_i L_i is enqueued on `commit_slot` from the SAME uploaded copy (one H2D for both; _device: both read the caller's buffer).
 * Collect the commitment's partial with kzg_msm_g1_srs_end(ctx, commit_slot, NULL, NULL, out_xyzz) (len = 0: nothing was enqueued there, the partial
 * is the identity); proof_slot must not be begun again before that.  The lagrange_shard handle and (_device) the evaluations must stay valid and
 * untouched until _end / _abort of the proof and the end of the commitment. */
/* commit_slot == proof_slot: GROUPED -- the two MSMs of the blob (the evaluations and the quotient over the same shard) leave as ONE batched launch
 * of the MSM engine from _continue (shard-sized MSMs are bound by dependent latency: two per launch cost 0.33 ms where two launches cost 0.46 at 2^17 pairs);
 * one slot per blob, so four blobs may be in flight.  Needs the shard's per-bit tables (kzg_srs_has_bit_tables(shard, 1) builds them for a shard of
 * fewer than 2^11 points) and kzg_msm_batch_capacity(len) >= 2 (slices of up to 2^18 elements), else KZG_ERR_INVALID_ARG.  Collect BOTH partial sums with kzg_commit_and_prove_lagrange_end (kzg_compute_proof_lagrange_end refuses a
 * grouped slot). */
int32_t kzg_commit_and_prove_lagrange_end(kzg_ctx* ctx, int32_t slot, uint64_t out_commit_xyzz_mont[16], uint64_t out_part[32]);
int32_t kzg_commit_and_prove_lagrange_begin(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const uint64_t* evals_slice_mont, size_t len,
                                            size_t n, const uint64_t z_mont[4], int32_t commit_slot, int32_t proof_slot);
int32_t kzg_commit_and_prove_lagrange_begin_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const void* d_evals_slice_mont, size_t len,
                                                   size_t n, const uint64_t z_mont[4], int32_t commit_slot, int32_t proof_slot);
int32_t kzg_compute_proof_lagrange_partial_y(kzg_ctx* ctx, int32_t slot, uint64_t out_ypart_mont[8]);
int32_t kzg_compute_proof_lagrange_continue(kzg_ctx* ctx, int32_t slot, const uint64_t y_mont[4]);
int32_t kzg_compute_proof_lagrange_end(kzg_ctx* ctx, int32_t slot, uint64_t out_part[32]);
int32_t kzg_compute_proof_lagrange_abort(kzg_ctx* ctx, int32_t slot);
int32_t kzg_lagrange_fold_y(const uint64_t* yparts_mont, size_t count, size_t n, const uint64_t z_mont[4], uint64_t out_y_mont[4]);
/* KZG::compute_quotient_eval_on_domain (prover/src/kzg.rs:237-260): sum over the n roots w^i != z of (f_i - value) w^i / ((z - w^i) z), i.e. the
 * quotient's evaluation AT the domain point z = w^m when value = f_m; like the reference, z need not be a domain point (then no term is skipped).
 * n evaluations in host memory, n a power of two (else KZG_ERR_NOT_POWER_OF_TWO; n > 2^28 -> KZG_ERR_DOMAIN); z = 0 -> KZG_ERR_INVALID_ARG (the
 * reference divides by z).  Computed on the GPU by the kernels of the Lagrange-sharded proof (csrc/lagrange.hip) on slot 0, which must be idle. */
int32_t kzg_compute_quotient_eval_on_domain(kzg_ctx* ctx, const uint64_t z_mont[4], const uint64_t* evals_mont, size_t n, const uint64_t value_mont[4],
                                            uint64_t out_quotient_mont[4]);
int32_t kzg_lagrange_fold_proof(const uint64_t* parts, size_t count, size_t n, const uint64_t z_mont[4], uint64_t out_xy_mont[8],
                                uint8_t* out_is_infinity);
/* ---- several GPUs behind one handle (no torch, no RCCL) ------------------------------------------------------
 * One context, one resident SRS shard and one host thread per entry of device_ids (an id may appear more than once: several
 * contexts on one GPU).  Device g holds the SRS powers [g N / G, (g+1) N / G) and commits that slice of every polynomial; the G
 * partial sums are folded on the host.  Same results, same status codes as the single-GPU calls they mirror:
 *   kzg_multi_commit_coeff_form  KZG::commit_coeff_form  (prover/src/kzg.rs:107-125)
 *   kzg_multi_commit_eval_form   KZG::commit_eval_form   (kzg.rs:84-104; every device transforms the whole polynomial)
 *   kzg_multi_compute_proof      KZG::compute_proof      (kzg.rs:215-234; the O(n) field work is done redundantly per device) */
typedef struct kzg_multi kzg_multi;
int32_t kzg_multi_create(const int32_t* device_ids, int32_t n_devices, kzg_multi** out);
void kzg_multi_destroy(kzg_multi* m);
int32_t kzg_multi_device_count(const kzg_multi* m);
size_t kzg_multi_srs_len(const kzg_multi* m);
int32_t kzg_multi_srs_upload(kzg_multi* m, const uint64_t* g1_xy_mont, size_t n_points);
int32_t kzg_multi_srs_generate(kzg_multi* m, const uint64_t tau_mont[4], size_t n_points);        /* known-tau SRS (tests, bench) */
/* One-time set-up for BASELINE config 4 WITHOUT replicated work: the Lagrange basis of the first n powers (KZG::g1_ifft, kzg.rs:263-285),
 * sharded by evaluation index (device g keeps L_i, i in [g n / G, (g+1) n / G), with its own tables).  From then on
 * kzg_multi_commit_eval_form / kzg_multi_compute_proof of exactly n evaluations make every device read, invert and divide ITS slice of the
 * caller's buffer only (csrc/lagrange.hip): no whole-polynomial upload, IFFT or quotient per device.  Same results.  Replaced by the next
 * kzg_multi_srs_upload / _generate. */
int32_t kzg_multi_cache_lagrange(kzg_multi* m, size_t n);
int32_t kzg_multi_commit_coeff_form(kzg_multi* m, const uint64_t* coeffs_mont, size_t n, uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
int32_t kzg_multi_commit_eval_form(kzg_multi* m, const uint64_t* evals_mont, size_t n, uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
int32_t kzg_multi_compute_proof(kzg_multi* m, const uint64_t* evals_mont, size_t n, size_t n_roots, const uint64_t z_mont[4],
                                uint64_t out_xy_mont[8], uint8_t* out_is_infinity, uint64_t* out_y_mont);
/* Resident inputs and streams (a commitment service; what `bench.py --multi` times): kzg_multi_scalars_upload keeps the slice
 * [g N / G, (g+1) N / G) of polynomial `buffer_id` (0 .. 15, n coefficients) in the HBM of device g; kzg_multi_commit_resident_stream
 * commits `count` of the uploaded polynomials (buffer_ids[k]) -- every device runs its own software pipeline over the stream (two
 * or three MSMs in flight, the asynchronous slots of kzg_msm_g1_srs_device_begin), the count x G partial sums are folded on the
 * host -- and writes count affine points. */
int32_t kzg_multi_scalars_upload(kzg_multi* m, int32_t buffer_id, const uint64_t* coeffs_mont, size_t n);
int32_t kzg_multi_commit_resident_stream(kzg_multi* m, const int32_t* buffer_ids, size_t count, uint64_t* out_xy_mont,
                                         uint8_t* out_is_infinity);

/* ---- one process per GPU: the exchanges over RCCL, behind the C-ABI (BASELINE north_star) -----------------------------------
 * RCCL has no reduction operator for elliptic-curve addition, so the "all-reduce" of the G partial sums is ONE all-gather of G small rows
 * over xGMI and a fold of G points on every rank.  Every rank of the communicator must make the same call (they are collectives).
 *   kzg_rccl_allgather_fold        partial in -> the same folded affine point on every rank
 *   kzg_commit_coeff_form_rccl     KZG::commit_coeff_form (prover/src/kzg.rs:107-125): this rank's resident coefficient slice over its shard of the
 *                                  monomial SRS + the exchange + the fold
 *   kzg_commit_eval_form_rccl      KZG::commit_eval_form (kzg.rs:84-104), BASELINE config 4's commitment: this rank's slice of the EVALUATIONS
 *                                  over its shard of the Lagrange basis (kzg_srs_lagrange_shard) + the exchange + the fold
 *   kzg_compute_proof_rccl         KZG::compute_proof_impl (kzg.rs:128-178, :237-260), config 4's proof, from the same slice: two exchanges
 *                                  (G x 72 B: partial barycentric sums -> y;  G x 264 B: partial points) -- the four steps of
 *                                  kzg_compute_proof_lagrange_* with the collectives in between; out_y (optional) = p(z)
 *   (_device: the slice is already in device memory and is read in place)
 * nccl_comm = the caller's ncclComm_t for this context's device.  The library uses the RCCL that is already in the process (the one that
 * made the communicator), else loads /opt/rocm/lib/librccl.so (KZG_RCCL_LIB overrides); no link-time dependency.  `world` must equal
 * ncclCommCount(comm) (checked: KZG_ERR_INVALID_ARG).
 * FAILURES.  A rank whose local work fails still issues every collective of the call with a poisoned row and then returns its own
 * status; every other rank returns KZG_ERR_PEER (kzg_ctx_last_error names the failed ranks): no rank is left blocked.  A peer that never
 * arrives: the wait is bounded by KZG_EXCHANGE_TIMEOUT_S seconds (default 60) -> KZG_ERR_EXCHANGE_TIMEOUT; exit, the communicator is
 * unusable.  Python hosts use torch.distributed instead (sharding.py: the same rows through PyTorch's communicator); one process driving
 * all GPUs uses kzg_multi_* (no collective). */
int32_t kzg_rccl_allgather_fold(kzg_ctx* ctx, void* nccl_comm, int32_t world, const uint64_t partial_xyzz_mont[16],
                                uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
int32_t kzg_commit_coeff_form_rccl(kzg_ctx* ctx, const kzg_srs* srs_shard, const void* d_coeffs_shard_mont, size_t n_shard, void* nccl_comm,
                                   int32_t world, uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
int32_t kzg_commit_eval_form_rccl(kzg_ctx* ctx, const kzg_srs* lagrange_shard, const uint64_t* evals_slice_mont, size_t len, void* nccl_comm,
                                  int32_t world, uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
int32_t kzg_commit_eval_form_rccl_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, const void* d_evals_slice_mont, size_t len, void* nccl_comm,
                                         int32_t world, uint64_t out_xy_mont[8], uint8_t* out_is_infinity);
int32_t kzg_compute_proof_rccl(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const uint64_t* evals_slice_mont, size_t len, size_t n,
                               const uint64_t z_mont[4], void* nccl_comm, int32_t world, uint64_t out_xy_mont[8], uint8_t* out_is_infinity,
                               uint64_t* out_y_mont);
int32_t kzg_compute_proof_rccl_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const void* d_evals_slice_mont, size_t len, size_t n,
                                      const uint64_t z_mont[4], void* nccl_comm, int32_t world, uint64_t out_xy_mont[8], uint8_t* out_is_infinity,
                                      uint64_t* out_y_mont);

/* helpers::validate_g1_point (helpers.rs:694-708): KZG_OK, or KZG_ERR_G1_NOT_ON_CURVE (y^2 != x^3 + 3; the identity = all zeros is accepted, the
 * cofactor of G1 is 1 so there is no subgroup check to make).  Host-only. */
int32_t kzg_validate_g1_point(const uint64_t xy_mont[8]);
/* helpers::hash_to_field_element (helpers.rs:382-390): SHA-256 of msg, read big-endian, mod r.  Host-only. */
int32_t kzg_hash_to_field_element(const uint8_t* msg, size_t len, uint64_t out_mont[4]);
/* NOTE on the two Fiat-Shamir transcripts below (kzg_compute_challenge, kzg_compute_r_powers): their byte layout follows the reference
 * line by line, but the 32-byte compressed G1 encoding inside them (x little-endian, 0x80 = larger y, 0x40 = infinity) is ark-serialize's
 * `serialize_compressed`, RESTATED here and in oracle/ alike and pinned by NO vector the reference holds -- its own tests only check that the
 * functions are deterministic (primitives/tests/helpers_test.rs:846-949).  Everything else in this header is pinned by reference fixtures.
 *
 * helpers::compute_challenge (primitives/src/helpers.rs:411-472): the Fiat-Shamir evaluation point of a blob,
 *   z = SHA-256( "EIGENDA_FSBLOBVERIFY_V1_" || u64be(n) || n x 32 B evaluations (big-endian, canonical) || commitment ) mod r,
 * n = next_pow2(ceil(len / 32)); evaluations = the blob's 32-byte big-endian chunks mod r (Blob::to_polynomial_eval_form, last
 * chunk right-padded with zeros, zero elements up to n); commitment = ark-serialize compressed G1Affine (32 B, x little-endian,
 * flags in the top bits of the last byte).  Host only (x86 SHA extensions when present); the commitment must be on the curve
 * (helpers::validate_g1_point, helpers.rs:694-708): else KZG_ERR_G1_NOT_ON_CURVE. */
int32_t kzg_compute_challenge(const uint8_t* blob_bytes, size_t len, const uint64_t commitment_xy_mont[8], uint64_t out_z_mont[4]);
/* KZG::compute_blob_proof (prover/src/kzg.rs:288-309): validate the commitment, z = compute_challenge(blob, commitment),
 * proof = compute_proof_impl(blob.to_polynomial_eval_form(), z, srs).  n_roots = KZG::expanded_roots_of_unity.len()
 * (KZG_ERR_ROOTS_LENGTH when it differs from the padded blob length, kzg.rs:135-139).  Bytes in, point out: the blob crosses
 * PCIe once; its transcript hash runs on a host thread beside the upload / bytes->Fr kernels.  out_z_mont / out_y_mont
 * (optional) receive the challenge and p(z). */
int32_t kzg_compute_blob_proof(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, size_t n_roots,
                               const uint64_t commitment_xy_mont[8], uint64_t out_proof_xy_mont[8], uint8_t* out_is_infinity,
                               uint64_t* out_z_mont, uint64_t* out_y_mont);
/* KZG::commit_blob (kzg.rs:182-185) followed by KZG::compute_blob_proof (kzg.rs:288-309) on the same blob in one call: the
 * transcript prefix (tag, length, evaluations: everything but the commitment) is hashed on a host thread WHILE the GPU computes
 * the commitment, and finalised with the 32 commitment bytes; then the proof.  Same results as the two separate calls. */
int32_t kzg_commit_and_prove_blob(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, size_t n_roots,
                                  uint64_t out_commitment_xy_mont[8], uint8_t* out_commitment_is_infinity,
                                  uint64_t out_proof_xy_mont[8], uint8_t* out_proof_is_infinity,
                                  uint64_t* out_z_mont, uint64_t* out_y_mont);
/* ---- the batched prover: many proofs in one call (no counterpart in the reference, which proves one polynomial per call) ------------------
 * A proof is the commitment of the quotient's evaluations over the Lagrange basis (kzg.rs:176-177), so the proofs of `count` polynomials of
 * one length are ONE bucket problem, as the commitments of kzg_commit_eval_form_batch are; in front of it one fused kernel (one workgroup per
 * polynomial of up to 2^12 evaluations) computes y = f(z) and the quotient row with one inversion per polynomial, z on the domain included
 * (kzg.rs:237-260 without a search for the index: the lane that meets the zero denominator knows it).  Polynomials of more than 2^12
 * evaluations take the single-proof path inside the call.  The SRS handle is not const: the Lagrange basis of each length and its per-bit
 * tables are attached on first use, as for the batched commitments.  SLOTS: the batched MSM runs on the context's slots; a kzg_*_begin in
 * flight gives KZG_ERR_INVALID_ARG.  The work goes through GROUPS of rows whose device workspace fits kzg_ctx_set_prove_group_bytes
 * (0 = 256 MiB; a group is never smaller than one row); the results do not depend on it.
 *
 * kzg_compute_proof_batch: KZG::compute_proof (kzg.rs:128-178, :215-234, :237-260) for row b of evals_mont (count x n wire elements) at
 * zs_mont[b]: out_proofs_xy_mont[b] (8 words; the identity as zeros with out_is_infinity[b] = 1) and out_ys_mont[b] = f_b(z_b) equal
 * kzg_compute_proof on that row, bit for bit.  out_is_infinity and out_ys_mont may be NULL.  There is NO n_roots argument: the roots-length
 * check of kzg.rs:135-139 has no batch counterpart (the domain is the canonical one of n points).  Checks, in this order: a null handle, an
 * SRS of another context, out_proofs_xy_mont NULL: KZG_ERR_INVALID_ARG; count = 0: KZG_OK, nothing written; evals_mont or zs_mont NULL:
 * KZG_ERR_INVALID_ARG; n = 0 or no power of two: KZG_ERR_INVALID_INPUT_LENGTH (helpers.rs:485-487); n > 2^28 or count x n > 2^40:
 * KZG_ERR_TOO_LARGE; n > the SRS: KZG_ERR_SRS_CAPACITY_EXCEEDED (kzg.rs:89-94).  _device: the evaluations are resident (complete before the call). */
int32_t kzg_compute_proof_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* evals_mont, size_t n, size_t count, const uint64_t* zs_mont,
                                uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity, uint64_t* out_ys_mont);
int32_t kzg_compute_proof_batch_device(kzg_ctx* ctx, kzg_srs* srs, const void* d_evals_mont, size_t n, size_t count, const uint64_t* zs_mont,
                                       uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity, uint64_t* out_ys_mont);
/* kzg_compute_blob_proof_batch: KZG::compute_blob_proof (kzg.rs:288-309) for `count` blobs of any mix of lengths: blob b is blob_lens[b] bytes
 * at blobs[b] with the commitment commitments_xy_mont[b].  Row b of every output equals kzg_compute_blob_proof on blob b (with the roots of its
 * own padded length), bit for bit; out_is_infinity, out_zs_mont, out_ys_mont may be NULL.  The blobs are sorted into length classes (one per
 * log2 of the padded length); per class and group the bytes go up once, bytes -> Fr (helpers::to_fr_array) runs on the device beside the
 * transcripts on the host pool (exactly helpers::compute_challenge's bytes, helpers.rs:411-455), then the fused kernel and the batched MSM.
 * ERRORS are those of the single call, checked per blob BEFORE any device work in this order: a length without bytes KZG_ERR_INVALID_ARG;
 * more than 2^28 elements KZG_ERR_TOO_LARGE (polynomial.rs:42-46); a commitment off the curve KZG_ERR_G1_NOT_ON_CURVE (kzg.rs:295); an empty
 * blob KZG_ERR_ZERO_LENGTH (helpers.rs:554-558: no roots of unity exist for it, where the single call compares lengths, kzg.rs:135-139); a
 * padded length beyond the SRS KZG_ERR_SRS_CAPACITY_EXCEEDED (kzg.rs:89-94).  The call returns the status of the FIRST failing blob in index
 * order and writes its index to *out_bad_index (may be NULL; untouched on success).  In front of them: a null handle, an SRS of another
 * context, out_proofs_xy_mont NULL: KZG_ERR_INVALID_ARG; count = 0: KZG_OK, nothing written; blobs, blob_lens or commitments_xy_mont NULL:
 * KZG_ERR_INVALID_ARG. */
int32_t kzg_compute_blob_proof_batch(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* const* blobs, const size_t* blob_lens, const uint64_t* commitments_xy_mont,
                                     size_t count, uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity, uint64_t* out_zs_mont, uint64_t* out_ys_mont,
                                     size_t* out_bad_index);
/* kzg_commit_and_prove_blob_batch: the same with the commitments computed by the call (KZG::commit_blob, kzg.rs:182-185, as one batched MSM
 * per group over the same Lagrange basis, then kzg.rs:288-309): row b equals kzg_commit_and_prove_blob on blob b, bit for bit.
 * out_commitments_xy_mont (count x 8) is required; out_commitment_is_infinity and the optional outputs above may be NULL. */
int32_t kzg_commit_and_prove_blob_batch(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* const* blobs, const size_t* blob_lens, size_t count,
                                        uint64_t* out_commitments_xy_mont, uint8_t* out_commitment_is_infinity, uint64_t* out_proofs_xy_mont,
                                        uint8_t* out_proof_is_infinity, uint64_t* out_zs_mont, uint64_t* out_ys_mont, size_t* out_bad_index);
/* the device-workspace budget of a group of the batched prover, in bytes; 0 = the default (256 MiB) */
int32_t kzg_ctx_set_prove_group_bytes(kzg_ctx* ctx, size_t bytes);
/* The same as a STREAM (round 6): KZG::commit_blob + KZG::compute_blob_proof (kzg.rs:182-185, :288-309) of many blobs with up to
 * KZG_BLOB_JOBS of them in flight per context.  One call above is bound by ITS transcript -- SHA-256 over the whole blob is one
 * sequential stream, 14-15 ms per 32 MiB on a core with SHA extensions, against ~2.9 ms of GPU work -- but the transcripts of different
 * blobs are independent:
 *   _begin(job)  starts the job's transcript prefix (helpers.rs:411-455: everything but the commitment) on a host thread of its own and
 *                enqueues upload, bytes -> Fr and the commitment on one of the context's slots; returns without waiting for either.
 *                commitment_xy_mont != NULL: KZG::compute_blob_proof as it stands -- the caller's commitment is validated (kzg.rs:295,
 *                KZG_ERR_G1_NOT_ON_CURVE) and absorbed, none is computed.
 *   _end(job)    returns the job's commitment, proof, z and y (any out pointer may be NULL); waits for whatever is still missing.
 * EVERY begin / end call also moves every other job on as far as it can go without waiting (commitment collected -> 32 bytes appended
 * to its finished prefix -> z -> proof enqueued), so with `begin(k + d); end(k)` in a loop the hashes of d blobs run side by
 * side and the GPU works through commitments and proofs back to back: 2.9-3.1 ms per 32 MiB blob at d = 12 (3.1 at d = 8) instead of 16-17.  Results are bit-identical to
 * kzg_commit_and_prove_blob / kzg_compute_blob_proof.  Same argument checks and statuses as those; blobs of up to 2^24 elements.
 * LIFETIME: blob_bytes is read by the transcript thread until the job's _end call returns.  SLOTS: the jobs take the context's
 * KZG_NUM_SLOTS slots phase by phase (a slot still held by another kzg_*_begin call of the caller is left alone; the synchronous calls,
 * which run on slot 0, return KZG_ERR_INVALID_ARG while a job holds it -- collect the jobs first).  A failed job reports its status from
 * _end and is idle afterwards.  kzg_ctx_destroy joins whatever is still in flight. */
#ifndef KZG_BLOB_JOBS
#define KZG_BLOB_JOBS 16
#endif
int32_t kzg_commit_and_prove_blob_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, size_t n_roots,
                                        const uint64_t* commitment_xy_mont, int32_t job);
int32_t kzg_commit_and_prove_blob_end(kzg_ctx* ctx, int32_t job, uint64_t* out_commitment_xy_mont, uint8_t* out_commitment_is_infinity,
                                      uint64_t* out_proof_xy_mont, uint8_t* out_proof_is_infinity, uint64_t* out_z_mont, uint64_t* out_y_mont);
/* helpers::evaluate_polynomial_in_evaluation_form (helpers.rs:475-535) on the domain of size n. */
int32_t kzg_evaluate_polynomial_in_evaluation_form(kzg_ctx* ctx, const uint64_t* evals_mont, size_t n,
                                                   const uint64_t z_mont[4], uint64_t out_y_mont[4]);
/* helpers::calculate_roots_of_unity (helpers.rs:553-589): out receives next_pow2(ceil(len/32)) elements
 * (capacity `cap` elements); *n_out = count. */
int32_t kzg_calculate_roots_of_unity(kzg_ctx* ctx, uint64_t length_of_data_after_padding,
                                     uint64_t* out_mont, size_t cap, size_t* n_out);

/* ---- verifier surface ------------------------------------------------------------
 * G2 wire format: 16 u64 = x.c0 | x.c1 | y.c0 | y.c1, each a 4 x u64 Montgomery Fq (arkworks' Fq2{c0,c1} in memory);
 * identity = all zeros.  The pairing itself is O(1) per verification and runs on the host (optimal ate Miller loop + final
 * exponentiation, the construction arkworks computes; csrc/host_pairing.h); the n-point linear combinations and the n barycentric
 * evaluations of batch verification run on the GPU.  g2_tau_mont = NULL selects consts::G2_TAU (primitives/src/consts.rs:55-64). */
int32_t kzg_g2_generator(uint64_t out_g2_mont[16]);                  /* G2Affine::generator() */
int32_t kzg_g2_tau_mainnet(uint64_t out_g2_mont[16]);                /* consts::G2_TAU */
int32_t kzg_g2_mul_generator(const uint64_t scalar_mont[4], uint64_t out_g2_mont[16]);   /* [s]G2 (tests / custom setups) */
/* helpers::is_on_curve_g2 (helpers.rs:263-285): y^2 = x^3 + 3 / (9 + u) on the twist; the identity counts as on the curve.  Host-only. */
int32_t kzg_g2_is_on_curve(const uint64_t g2_mont[16], int32_t* out_on_curve);
/* helpers::example_validate_g2_point (helpers.rs:740-766), checks in the reference's order: *out_reason = 0 valid | 1 NotOnCurveError("G2 point not on
 * curve") | 2 NotOnCurveError("G2 point is point at infinity") | 3 NotOnCurveError("G2 point not in correct subgroup") ([r]P != O) |
 * 4 G2GeneratorNotAcceptedError("G2 point cannot be the generator point").  Host-only. */
int32_t kzg_validate_g2_point(const uint64_t g2_mont[16], int32_t* out_reason);
/* helpers::pairings_verify(a1, a2, b1, b2) (helpers.rs:392-398): *out_ok = (e(a1,a2) == e(b1,b2)).  Host-only. */
int32_t kzg_pairings_verify(const uint64_t a1_xy_mont[8], const uint64_t a2_g2_mont[16],
                            const uint64_t b1_xy_mont[8], const uint64_t b2_g2_mont[16], int32_t* out_ok);
/* verify::verify_proof (verifier/src/verify.rs:10-72).  Off-curve commitment/proof -> KZG_ERR_G1_NOT_ON_CURVE;
 * [tau - z]G2 == identity -> KZG_ERR_TAU_EQUALS_Z.  Host-only.
 * g2_tau (here and in kzg_verify_kzg_proof_batch): NULL = consts::G2_TAU; a caller-supplied point is only checked to be ON THE
 * CURVE, exactly as the reference does (verify.rs:29-33, batch.rs:212-214) -- its membership in the order-r subgroup of the twist
 * is NOT checked; outside that subgroup a pairing value is not defined by the reference either (a degenerate Miller-loop step,
 * T = +-Q, makes this library answer "not equal"): pass subgroup points (any [s]G2). */
int32_t kzg_verify_proof(const uint64_t commitment_xy_mont[8], const uint64_t proof_xy_mont[8],
                         const uint64_t value_mont[4], const uint64_t z_mont[4],
                         const uint64_t* g2_tau_mont, int32_t* out_ok);
/* verify::verify_blob_kzg_proof (verifier/src/verify.rs:76-98) in one call: both points validated (KZG_ERR_G1_NOT_ON_CURVE), the blob's
 * challenge z = compute_challenge(blob, commitment) (helpers.rs:411-472, host SHA-256), y = p(z) (helpers.rs:475-535, GPU), then
 * verify_proof above.  blob_bytes = the padded bytes of the blob (Blob::data()); an empty blob -> KZG_ERR_ZERO_LENGTH. */
int32_t kzg_verify_blob_kzg_proof(kzg_ctx* ctx, const uint8_t* blob_bytes, size_t len, const uint64_t commitment_xy_mont[8],
                                  const uint64_t proof_xy_mont[8], const uint64_t* g2_tau_mont, int32_t* out_ok);
/* batch::verify_kzg_proof_batch (verifier/src/batch.rs:185-256) after the caller has derived r_powers from its
 * transcript (compute_r_powers, batch.rs:76-168): point validation, the three g1_lincomb calls as one batched GPU MSM,
 * the final 2-pairing check. */
int32_t kzg_verify_kzg_proof_batch(kzg_ctx* ctx, const uint64_t* commitments_xy_mont, const uint64_t* zs_mont,
                                   const uint64_t* ys_mont, const uint64_t* proofs_xy_mont,
                                   const uint64_t* r_powers_mont, size_t n,
                                   const uint64_t* g2_tau_mont, int32_t* out_ok);
/* batch::compute_r_powers (verifier/src/batch.rs:76-168): r = SHA-256("EIGENDA_RCKZGBATCH___V1_" || 8 zero bytes || u64be(n) ||
 * n x u64be(blobs_as_field_elements_length[i]) || n x (C_i || z_i || y_i || proof_i)) mod r with the points ark-compressed and z, y
 * canonical big-endian; out = [r^0 .. r^(n-1)] (helpers::compute_powers, helpers.rs:298-313).  Host only (rows serialised on a
 * thread pool). */
int32_t kzg_compute_r_powers(const uint64_t* commitments_xy_mont, const uint64_t* zs_mont, const uint64_t* ys_mont,
                             const uint64_t* proofs_xy_mont, const uint64_t* blobs_as_field_elements_length, size_t n,
                             uint64_t* out_r_powers_mont);
/* helpers::compute_challenges_and_evaluate_polynomial (primitives/src/helpers.rs:613-662) for n blobs in ONE call:
 * out_zs[i] = compute_challenge(blob_i, commitment_i) (helpers.rs:411-472), out_ys[i] = p_i(z_i) (helpers.rs:475-535).
 * blobs[i] / blob_lens[i] = the padded bytes of blob i (Blob::data()).  The n transcripts are hashed on a pool of host threads
 * (KZG_HOST_THREADS_MAX, default min(48, hardware threads, the cgroup's CPU quota)); the n barycentric evaluations run as one batched GPU launch for blobs of up to
 * 4096 field elements (one workgroup per blob, one inversion per blob) and through the single-polynomial path beyond.  Errors, for
 * the first failing blob in order: KZG_ERR_TOO_LARGE (polynomial.rs:42-46), KZG_ERR_G1_NOT_ON_CURVE (helpers.rs:413),
 * KZG_ERR_ZERO_LENGTH (empty blob: helpers.rs:554-558). */
int32_t kzg_compute_challenges_and_evaluate_polynomial(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* blob_lens,
                                                       const uint64_t* commitments_xy_mont, size_t n,
                                                       uint64_t* out_zs_mont, uint64_t* out_ys_mont);
/* The evaluation half of the call above with the points given: out_ys[i] = p_i(zs[i]) for n blobs (helpers.rs:475-535 each, incl.
 * the early return for z on the domain, helpers.rs:497-504), one batched GPU launch.  KZG_ERR_TOO_LARGE / KZG_ERR_ZERO_LENGTH as above. */
int32_t kzg_evaluate_blobs_in_evaluation_form_batch(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* blob_lens,
                                                    const uint64_t* zs_mont, size_t n, uint64_t* out_ys_mont);
/* batch::verify_blob_kzg_proof_batch (verifier/src/batch.rs:16-69) end to end -- BASELINE config 5 in one call: validation of the
 * 2n points (KZG_ERR_G1_NOT_ON_CURVE), the n challenges and evaluations (above), compute_r_powers, then verify_kzg_proof_batch
 * (three batched GPU MSMs + the host 2-pairing check).  *out_ok = 1 iff every proof verifies.  n = 0 -> *out_ok = 1. */
int32_t kzg_verify_blob_kzg_proof_batch(kzg_ctx* ctx, const uint8_t* const* blobs, const size_t* blob_lens,
                                        const uint64_t* commitments_xy_mont, const uint64_t* proofs_xy_mont, size_t n,
                                        const uint64_t* g2_tau_mont, int32_t* out_ok);

/* ---- verification of coset proofs (the proofs of kzg_compute_multiproofs; the reference has none) -------------------------------
 * n = domain size, w its primitive n-th root, l = chunk_len, m = n / l.  Coset k < m is {w^(k + j m) : j < l}; its values
 * ys[j] = f(w^(k + j m)) are evals[k::m], its proof pi_k = [f / (X^l - w^(k l))](tau) G1 is entry k of kzg_compute_multiproofs.  With
 * I_k the polynomial of degree < l through the values, I_k(X) = sum_t w^(-k t) IFFT_l(ys)_t X^t (IFFT_l over the root w^m, natural
 * order), one proof verifies iff e(pi_k, [tau^l]_2 - [w^(k l)]G2) = e(C - [I_k(tau)]_1, G2).  A batch of N items (item i: commitment
 * row c_i of M commitments, coset k_i, l values, proof pi_i) with weights r_i is ONE pairing check whatever N is:
 *     A_t = sum_i r_i w^(-k_i t) IFFT_l(ys_i)_t                                  (GPU, kzg_coset_interpolate_rlc)
 *     e(sum_i r_i pi_i, [tau^l]_2) = e(sum_rows (sum_{i: c_i = row} r_i) C_row - sum_t A_t [tau^t]_1 + sum_i r_i w^(k_i l) pi_i, G2)
 * (for l = 1 the equation of kzg_verify_kzg_proof_batch).  The verifier needs the first l G1 points of an SRS and one G2 point.
 *
 * kzg_coset_interpolate_rlc: out[t] = sum_i weights[i] * w^(-coset_indices[i] * t) * IFFT_l(ys_i)[t].  ys: count x chunk_len x 4 u64,
 * coset_indices: count values < n / chunk_len, weights: count x 4 u64, out: chunk_len x 4 u64 (canonical wire words: equal inputs give
 * equal bits whatever the launch geometry).  Device memory grows with count * chunk_len only, not with n.  count = 0 -> zeros.
 * Errors: a null pointer (with count > 0) -> KZG_ERR_INVALID_ARG; n = 0 or not a power of two -> KZG_ERR_NOT_POWER_OF_TWO; n > 2^24 ->
 * KZG_ERR_DOMAIN; n = 1, chunk_len not a power of two or > n / 2, a coset index >= n / chunk_len -> KZG_ERR_INVALID_ARG;
 * count * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE. */
int32_t kzg_coset_interpolate_rlc(kzg_ctx* ctx, const uint64_t* ys_mont, const uint64_t* coset_indices, const uint64_t* weights_mont,
                                  size_t count, size_t n, size_t chunk_len, uint64_t* out_coeffs_mont);
/* The Fiat-Shamir weights [r^0 .. r^(count-1)] of a batch.  Host only.  This library's own transcript, built like the one of
 * kzg_compute_r_powers but in two levels, so that the count x chunk_len x 32 bytes of values are hashed on the host pool:
 *   d_i = SHA-256("KZGBN254_COSETITEM___V1_" || u64be(c_i) || u64be(k_i) || chunk_len x be32(ys_i[j]) || ark-compressed pi_i)
 *   r   = SHA-256("KZGBN254_COSETBATCH__V1_" || u64be(n) || u64be(chunk_len) || u64be(n_commitments) || u64be(count) ||
 *                 n_commitments x ark-compressed C || d_0 || .. || d_(count-1)) mod r
 * (both tags 24 bytes; point and scalar encodings as in kzg_compute_r_powers).  count = 0 writes nothing.  A null pointer ->
 * KZG_ERR_INVALID_ARG; count * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE.  Points are serialised as given, not validated. */
int32_t kzg_compute_multiproof_r_powers(const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                                        const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont,
                                        size_t count, size_t n, size_t chunk_len, uint64_t* out_r_powers_mont);
/* The same weights, bit for bit, with the count item digests hashed on the device: values, indices and proofs are uploaded, one lane per
 * item produces and hashes its 72 + 32 chunk_len bytes (csrc/coset_item_stream.h), the 32 count digest bytes come back, the one sequential
 * batch hash runs on the host, and r^i is one product of two table entries per lane.  Inputs the host entry does not validate -- a value
 * >= r, a coordinate >= p -- are detected on the device and that transcript is recomputed on the host, so every input gives the host entry's
 * bits.  Arguments and errors as above; a null ctx -> KZG_ERR_INVALID_ARG. */
int32_t kzg_compute_multiproof_r_powers_device(kzg_ctx* ctx, const uint64_t* commitments_xy_mont, size_t n_commitments,
                                               const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                               const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len,
                                               uint64_t* out_r_powers_mont);
/* The batch equation above: upload of values / indices / weights, kzg_coset_interpolate_rlc's kernels, an MSM of the l coefficients
 * over srs[0 .. l) with the scalars left on the device, the two count-point combinations of the proofs and the n_commitments-point
 * one of the commitments as batched MSMs (every uploaded point checked on the device), point sums and ONE pairing check on the host.
 * r_powers_mont = NULL derives the weights of kzg_compute_multiproof_r_powers: on the host pool, or (kzg_ctx_set_transcript_device) on the
 * device from the values uploaded for the interpolation, which then go up once.  The same item may appear twice.  *out_ok = 1 iff the
 * equation holds; a failed check is *out_ok = 0 with KZG_OK.  count = 0 -> *out_ok = 1.
 * g2_tau_l_mont = [tau^l]_2 in the G2 wire format, checked to be on the twist (not its subgroup: see kzg_verify_proof); NULL is
 * allowed for chunk_len = 1 only and then means consts::G2_TAU.  The identity (all-zero wire point) is a valid commitment and proof.
 * Errors, in this order: a null pointer (with count > 0), NULL g2_tau_l_mont with chunk_len != 1, srs of another context or a
 * Lagrange-basis handle -> KZG_ERR_INVALID_ARG; n = 0 or not a power of two -> KZG_ERR_NOT_POWER_OF_TWO; n > 2^24 -> KZG_ERR_DOMAIN;
 * n = 1, chunk_len not a power of two or > n / 2 -> KZG_ERR_INVALID_ARG; chunk_len > kzg_srs_len(srs) ->
 * KZG_ERR_SRS_CAPACITY_EXCEEDED; a coset index >= n / chunk_len or a commitment index >= n_commitments -> KZG_ERR_INVALID_ARG;
 * count * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE; a commitment or proof off the curve -> KZG_ERR_G1_NOT_ON_CURVE; then g2_tau_l_mont off
 * the twist -> KZG_ERR_G2_TAU_NOT_ON_CURVE. */
int32_t kzg_verify_multiproof_batch(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments,
                                    const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                    const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len,
                                    const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, int32_t* out_ok);
/* ---- batches of MIXED shapes: one call, one product of pairings ----------------------------------------------------------------
 * A batch has n_classes shape classes; class s is the pair (n_s, l_s) = (class_n[s], class_chunk_len[s]) with m_s = n_s / l_s cosets and
 * w_s the primitive n_s-th root of the library; the rules for a class are those of n / chunk_len above.  Item i has the class
 * s_i = class_indices[i], a commitment row c_i, a coset k_i < m_{s_i}, l_{s_i} values and a proof.  Only the G2 side of the equation
 * depends on the chunk length, and the interpolation polynomials of all shapes add into one coefficient vector:
 *     A_t = sum_{i : l_{s_i} > t} r_i w_{s_i}^(-k_i t) IFFT_{l_{s_i}}(ys_i)_t          t < l_max          (GPU, kzg_coset_interpolate_rlc_mixed)
 *     L_d = sum_{i : l_{s_i} = d} r_i pi_i                                             one per DISTINCT chunk length d
 *     R   = sum_i r_i C_{c_i} - sum_t A_t [tau^t]_1 + sum_i r_i w_{s_i}^(k_i l_{s_i}) pi_i
 *     accept <=> prod_d e(L_d, [tau^d]_2) e(-R, G2) = 1
 * 1 + (distinct chunk lengths that have items) pairs whatever the item count; two classes of equal l and different n share a pair.  For one
 * class this is the equation of kzg_verify_multiproof_batch (whose transcript differs: a batch of ONE shape belongs there, see README).
 * Common arguments: class_n, class_chunk_len: n_classes u64 each; class_indices: count u64; ys_mont is RAGGED: item i's l_{s_i} values
 * follow item i - 1's, in the caller's item order, with no padding.  Items may come in any order; classes may be empty or repeated.
 *
 * kzg_coset_interpolate_rlc_mixed: out = the l_max coefficients A_t with r_i = weights[i], canonical wire words; l_max is the largest
 * class_chunk_len over ALL classes, empty ones included.  Equal inputs give equal bits whatever the item order, the class numbering or the
 * launch geometry.  count = 0 -> zeros.  Errors, in this order: a null pointer -> KZG_ERR_INVALID_ARG; n_classes = 0 with count > 0 ->
 * KZG_ERR_INVALID_ARG; n_classes > 512 -> KZG_ERR_TOO_LARGE; every class, in class order, by the table of kzg_coset_interpolate_rlc
 * (KZG_ERR_NOT_POWER_OF_TWO / KZG_ERR_DOMAIN / KZG_ERR_INVALID_ARG); a class index >= n_classes or a coset index >= m_{s_i} ->
 * KZG_ERR_INVALID_ARG; sum_i l_{s_i} > 2^28 -> KZG_ERR_TOO_LARGE. */
int32_t kzg_coset_interpolate_rlc_mixed(kzg_ctx* ctx, const uint64_t* class_n, const uint64_t* class_chunk_len, size_t n_classes,
                                        const uint64_t* class_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                        const uint64_t* weights_mont, size_t count, uint64_t* out_coeffs_mont);
/* The Fiat-Shamir weights [r^0 .. r^(count-1)] of a batch of mixed shapes.  Host only.  The item digest d_i is the one of
 * kzg_compute_multiproof_r_powers over c_i, k_i, the item's OWN l_{s_i} values and its proof; then
 *   r = SHA-256("KZGBN254_COSETMIXED__V1_" || u64be(n_classes) || n_classes x (u64be(n_s) || u64be(l_s)) || u64be(n_commitments) ||
 *               u64be(count) || count x u64be(s_i) || n_commitments x ark-compressed C || d_0 || .. || d_(count-1)) mod r
 * (the tag 24 bytes; encodings and the reduction as there).  count = 0 writes nothing.  A null pointer, a class index >= n_classes or a
 * chunk length 0 -> KZG_ERR_INVALID_ARG; sum_i l_{s_i} > 2^28 -> KZG_ERR_TOO_LARGE.  Points are serialised as given, not validated. */
int32_t kzg_compute_multiproof_r_powers_mixed(const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                                              const uint64_t* class_n, const uint64_t* class_chunk_len, size_t n_classes,
                                              const uint64_t* class_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                              const uint64_t* proofs_xy_mont, size_t count, uint64_t* out_r_powers_mont);
/* The mixed equation above: values, indices and weights go up once in the caller's order, the interpolation kernels (one launch for the
 * classes of l <= 512, one for l = 1024, one transform per coset above that) and a row sum leave the l_max coefficients on the device, ONE
 * MSM over srs[0 .. l_max), one variable-base MSM per distinct chunk length over the proofs (uploaded sorted by chunk length), one over
 * the second copy of the proofs and the commitments, and ONE pooled product of pairings on the host.  g2_tau_l_mont: n_classes G2 wire
 * points, entry s = [tau^{l_s}]_2, checked to be on the twist (classes that have items only); never NULL (there is no consts::G2_TAU
 * shortcut).  r_powers_mont = NULL derives the weights of kzg_compute_multiproof_r_powers_mixed on the host pool before the context is
 * taken.  *out_ok = 1 iff the equation holds; a failed equation is *out_ok = 0 with KZG_OK.  count = 0 -> *out_ok = 1, no device work.
 * Every chunk length kzg_verify_multiproof_batch accepts is accepted; the entry is refused while a kzg_*_begin is in flight.
 * Errors, in this order: (1) a null pointer, srs of another context or a Lagrange-basis handle -> KZG_ERR_INVALID_ARG; (2) n_classes = 0
 * with count > 0 -> KZG_ERR_INVALID_ARG; (3) n_classes > 512 -> KZG_ERR_TOO_LARGE; (4) every class, in class order, by the table of
 * kzg_verify_multiproof_batch for (n, chunk_len); (5) l_max > kzg_srs_len(srs) -> KZG_ERR_SRS_CAPACITY_EXCEEDED; (6) a class index >=
 * n_classes, a coset index >= m_{s_i} or a commitment index >= n_commitments -> KZG_ERR_INVALID_ARG; (7) sum_i l_{s_i} > 2^28 ->
 * KZG_ERR_TOO_LARGE; (8) two classes of equal chunk length whose G2 points differ bit-wise -> KZG_ERR_INVALID_ARG; (9) a commitment or
 * proof off the curve -> KZG_ERR_G1_NOT_ON_CURVE; (10) a G2 entry of a class that has items off the twist, in class order ->
 * KZG_ERR_G2_TAU_NOT_ON_CURVE. */
int32_t kzg_verify_multiproof_batch_mixed(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments,
                                          const uint64_t* commitment_indices, const uint64_t* class_n, const uint64_t* class_chunk_len,
                                          size_t n_classes, const uint64_t* class_indices, const uint64_t* coset_indices,
                                          const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t count,
                                          const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, int32_t* out_ok);
/* One proof: the batch of one item with weight 1 (ys: chunk_len x 4 u64).  Errors as kzg_verify_multiproof_batch. */
int32_t kzg_verify_multiproof(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t commitment_xy_mont[8], const uint64_t proof_xy_mont[8],
                              uint64_t coset_index, const uint64_t* ys_mont, size_t n, size_t chunk_len,
                              const uint64_t* g2_tau_l_mont, int32_t* out_ok);
/* Locating the bad items of a rejected batch.  The batch equation is linear in the set of items, so for ANY partition of the items into
 * n_groups groups (group_indices[i] < n_groups is item i's group; a group may be empty) the device produces, in one pass over the batch,
 * the two G1 sums of every group's own equation:
 *     L_g     = sum_{i in g} r_i pi_i
 *     A_{g,t} = sum_{i in g} r_i w^(-k_i t) IFFT_l(ys_i)_t
 *     R_g     = sum_{i in g} r_i C_{c_i} + sum_{i in g} r_i w^(k_i l) pi_i - sum_t A_{g,t} [tau^t]_1
 * Group g is good iff e(L_g, [tau^l]_2) = e(R_g, G2).  Summed over all groups (L, R) is exactly the pair kzg_verify_multiproof_batch
 * checks, so the verdict on the sum of all groups is that entry's verdict for the same inputs and weights.
 *
 * kzg_coset_group_sums: the arguments of kzg_verify_multiproof_batch without g2_tau_l_mont and out_ok, the partition, and the outputs
 * out_lhs_xy_mont / out_rhs_xy_mont (n_groups x 8 u64, affine G1 wire points, canonical words) with out_lhs_is_infinity /
 * out_rhs_is_infinity (n_groups bytes).  Equal inputs give equal bits, whatever the order of the items inside a group and whatever the
 * launch geometry.  An empty group gives the identity twice.  r_powers_mont = NULL derives the weights of
 * kzg_compute_multiproof_r_powers exactly as the batch entry does (device transcript and host fallback included).  The items are sorted
 * by group on the host as a permutation; the values go up once, in the caller's order.  The n_groups l-point MSMs run as one MSM problem
 * like kzg_commit_coeff_form_batch_device, and like that call an SRS without per-bit tables gets them on first use: srs is not const.
 * Errors, in this order: those of kzg_verify_multiproof_batch up to and including the check of coset and commitment indices (a null
 * group_indices or output counts as a null pointer); a group index >= n_groups, or n_groups = 0 with count > 0 -> KZG_ERR_INVALID_ARG;
 * count * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE; n_groups > 2^28 -> KZG_ERR_TOO_LARGE (before anything is allocated); a commitment or
 * proof off the curve -> KZG_ERR_G1_NOT_ON_CURVE.  KZG_ERR_INVALID_ARG also while a kzg_*_begin is in flight (the MSMs use the slots). */
int32_t kzg_coset_group_sums(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments,
                             const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                             const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len, const uint64_t* r_powers_mont,
                             const uint64_t* group_indices, size_t n_groups, uint64_t* out_lhs_xy_mont, uint8_t* out_lhs_is_infinity,
                             uint64_t* out_rhs_xy_mont, uint8_t* out_rhs_is_infinity);
/* The group sums above, then a search on the host: prefix sums of the groups' pairs in group order make the pair of any range of groups
 * a difference of two prefixes; the root is tested first; a range that holds marks all its groups good; a failing range of one group
 * marks it bad; any other failing range is halved and its left half tested (if that holds, the right half fails without a test).  Each
 * test is one pairing check (the pooled check of the batch entry) and no GPU work: at most 1 + 2 b ceil(log2 n_groups) checks for b bad
 * groups, and exactly one for a good batch.  out_group_ok: n_groups bytes, 1 = good; *out_bad_groups = the number of bad groups;
 * *out_pairing_checks (may be NULL) = the checks made.  KZG_OK with *out_bad_groups = 0 is the accept of kzg_verify_multiproof_batch.
 * Soundness: a range that holds could in principle hide two bad groups that cancel; with weights derived from the transcript over ALL
 * inputs (r_powers_mont = NULL, or kzg_compute_multiproof_r_powers) that has negligible probability, with weights of the caller's own
 * choosing there is no such guarantee.
 * This entry always pays for the group sums: a caller who expects good batches calls kzg_verify_multiproof_batch first and this one
 * only after a reject.  count = 0 -> every group good, no device work, no pairing check.
 * Pairing checks of a located batch on the DEVICE (kzg_ctx_set_locate_pairings(ctx, 1); mode 0, the default, is everything above,
 * unchanged).  The root is still tested on the host, so a good batch costs exactly one check and no further GPU work.  After a failing
 * root over S > 1 non-empty groups the equation e(lhs_g, [tau^l]_2) e(-rhs_g, G2) = 1 of EVERY such group is evaluated as one batch of
 * S two-pair checks on the device (the group sums made affine with one inversion per 256; kzg_pairings_product_verify_batch's kernel),
 * and the verdicts are out_group_ok.  A failing root over S = 1 names that group without another check.  *out_pairing_checks counts every
 * equation evaluated, on the host or on the device: 1 if the root holds or S <= 1, else 1 + S.  kzg_retrieve_blobs_bytes_tolerant runs
 * such a pass over the blobs and one over the decodable items of all bad blobs together: 1 (the batch equation) + on a reject
 * [1 + blobs, or 1 for a single blob] + [1 + I, or 1 for I = 1, nothing for I = 0] for I such items.  Leaf tests are exact where the
 * search's "a range that holds is all good" is statistical: the two modes give the same map except with the cancellation probability of
 * csrc/host_locate.h's note 3 (two bad groups cancelling inside a range that the search tests and mode 1 never forms).  The device pass
 * takes the time of one check per 64 x (SIMDs of the device) groups, about 24 ms (profiles/pairing_device.md), where the search pays
 * about 0.5 ms per check and the work between them: measured, mode 1 wins from three bad chunks among 64 x 513 on and loses at one.  Header locate (variable G2 points, 3 + lengths pairs per
 * group) keeps the host search in both modes.
 * Errors: those of kzg_coset_group_sums in its order (NULL g2_tau_l_mont with chunk_len != 1 where the batch entry reports it), then
 * g2_tau_l_mont off the twist -> KZG_ERR_G2_TAU_NOT_ON_CURVE. */
int32_t kzg_verify_multiproof_batch_locate(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments,
                                           const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                           const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len,
                                           const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, const uint64_t* group_indices,
                                           size_t n_groups, uint8_t* out_group_ok, size_t* out_bad_groups, size_t* out_pairing_checks);

/* ---- erasure decoding: a polynomial from a subset of its cosets ------------------------------------------------------------------
 * The cosets are those above: coset k < m = n / chunk_len is {w^(k + j m) : j < chunk_len}, its values ys[j] = f(w^(k + j m)) (row k
 * of KZG.cosets).  Given `count` DISTINCT cosets -- ys_mont: count x chunk_len x 4 u64, item i being the coset coset_indices[i], in any
 * order -- the call returns the unique polynomial f of degree < count * chunk_len through those values: out_poly_mont, n x 4 u64
 * canonical wire words, its evaluations on {w^i} (eval_form = 1) or its n coefficients (eval_form = 0; those from count * chunk_len on
 * are zero).  *out_consistent = 1 iff deg f < degree_bound, i.e. the values are those of a polynomial below that bound; a failed check
 * is 0 with KZG_OK and f is still the interpolant.  degree_bound = 0 means count * chunk_len (the flag is then always 1);
 * out_consistent may be NULL.  Synchronous, host buffers, no SRS.  Equal inputs give equal bits whatever the launch geometry and
 * whatever the order of the items.
 * Method: with M the missing cosets and Z(X) = prod_{k in M} (X^l - w^(l k)), f Z has degree < n and known values on the whole
 * domain (0 on M), so it is one IFFT; f is its quotient by Z on the shifted domain {5 w^i}: four transforms of n points (three for
 * coefficients), three pointwise passes, and the values of Z as DIRECT products, 2 m (m - count) field products.  That part is
 * quadratic in m, hence the last error below; the cap leaves every (n, chunk_len) with m <= 2^16 unrestricted and admits a larger m
 * with proportionally fewer missing cosets.  Device memory: n x 32 B of values, the transforms' workspace (n x 32 B above 2^10
 * points, 2 n x 32 B above 2^20, which also stages the upload), at most 80 m bytes of indices and vanishing values, at most 9 MiB of partial
 * products and 72 (2^10 + n / 2^10) bytes of powers of 5.  Nothing proportional to n is computed on the host.
 * Errors, checked on the host before any kernel runs, in this order: 1. a null pointer -> KZG_ERR_INVALID_ARG; 2. n = 0 or not a
 * power of two -> KZG_ERR_NOT_POWER_OF_TWO; 3. n > 2^24 -> KZG_ERR_DOMAIN; 4. n = 1, chunk_len not a power of two or > n / 2 ->
 * KZG_ERR_INVALID_ARG; 5. count = 0 or count > m -> KZG_ERR_INVALID_ARG; 6. an index >= m or a duplicate index ->
 * KZG_ERR_INVALID_ARG; 7. degree_bound > count * chunk_len (too few cosets) -> KZG_ERR_INVALID_ARG; 8. m * (m - count) > 2^32 ->
 * KZG_ERR_TOO_LARGE.  After any error the context stays usable. */
int32_t kzg_recover_from_cosets(kzg_ctx* ctx, const uint64_t* ys_mont, const uint64_t* coset_indices, size_t count, size_t n,
                                size_t chunk_len, size_t degree_bound, int32_t eval_form, uint64_t* out_poly_mont,
                                int32_t* out_consistent);
/* kzg_recover_from_cosets for `blobs` blobs of one shape (n, chunk_len, count, degree_bound, eval_form) in one call.  ys_mont: blobs x
 * count x chunk_len x 4 u64, blob b at ys_mont + b count chunk_len 4.  coset_indices: index_rows x count; index_rows = 1: every blob
 * has these cosets, in this order of items; index_rows = blobs: row b belongs to blob b.  Row b of out_polys_mont (blobs x out_len x 4)
 * and out_consistent[b] (may be NULL) are bit-identical to kzg_recover_from_cosets on blob b with its row of indices, whatever the
 * grouping, the launch geometry, the order of the items inside a blob and whichever other blobs share the call.
 * out_len: 0 means n.  With eval_form = 1 it must be 0 or n.  With eval_form = 0 any value with degree_bound (resolved: 0 -> count *
 * chunk_len) <= out_len <= n is allowed: only the first out_len coefficients of each blob are written and downloaded (a consistent blob
 * has nothing but zeros from degree_bound on); the rows are compacted on the device, the download is one contiguous copy.  The flag
 * still covers every coefficient from degree_bound to n.
 * The blobs' missing sets are deduplicated into patterns (a set, whatever the order of the items): the vanishing values are computed
 * once per pattern of a group, not once per blob.  The call works through the blobs in GROUPS whose device workspace fits a byte
 * budget (4 GiB unless kzg_ctx_set_recover_group_bytes says otherwise; at most 32 768 blobs; sized for the worst case of one pattern
 * per blob, so the grouping depends on the shape alone; never smaller than one blob): inside a group every stage is one launch for
 * all its blobs, with one upload of the values, one of indices and patterns, one download of the rows and one of the flags.
 * Synchronous, host buffers, no SRS.
 * Errors, checked on the host before any kernel runs, in this order:
 *   1. a null ctx, ys, indices or output, or blobs = 0 -> KZG_ERR_INVALID_ARG;
 *   2. index_rows neither 1 nor blobs -> KZG_ERR_INVALID_ARG;
 *   3. rows 2 .. 5 of kzg_recover_from_cosets' table, unchanged;
 *   4. an index >= m or a duplicate index in any row -> KZG_ERR_INVALID_ARG;
 *   5. degree_bound > count * chunk_len -> KZG_ERR_INVALID_ARG;
 *   6. a bad out_len -> KZG_ERR_INVALID_ARG;
 *   7. m * (m - count) > 2^32 -> KZG_ERR_TOO_LARGE;
 *   8. blobs x n x 32 bytes overflowing size_t -> KZG_ERR_INVALID_ARG.
 * After any error the context stays usable. */
int32_t kzg_recover_from_cosets_batch(kzg_ctx* ctx, const uint64_t* ys_mont /* blobs x count x chunk_len x 4 */,
                                      const uint64_t* coset_indices /* index_rows x count */, size_t index_rows, size_t blobs,
                                      size_t count, size_t n, size_t chunk_len, size_t degree_bound, int32_t eval_form,
                                      size_t out_len /* 0 = n */, uint64_t* out_polys_mont /* blobs x out_len x 4 */,
                                      int32_t* out_consistent /* blobs, may be NULL */);
/* The workspace budget of a group of kzg_recover_from_cosets_batch on this context, in bytes; 0 = the default (4 GiB). */
int32_t kzg_ctx_set_recover_group_bytes(kzg_ctx* ctx, size_t bytes);
/* How kzg_recover_from_cosets_batch groups these blobs: a pure query (no context, no device).  group_bytes: the budget, 0 = the
 * default.  Errors: out NULL or blobs = 0 -> KZG_ERR_INVALID_ARG, rows 3 of the table above, out_len > n -> KZG_ERR_INVALID_ARG, rows 7
 * and 8. */
typedef struct kzg_recover_batch_info_t {    /* (_t: the function below has the plain name, and C has one name space for both) */
    uint64_t blobs_per_group;            /* the last group of a call may hold fewer */
    uint64_t groups;
    uint64_t group_bytes;                /* device workspace of one full group, every blob with its own pattern */
    uint64_t blob_bytes;                 /* of which per blob */
} kzg_recover_batch_info_t;
int32_t kzg_recover_batch_info(size_t blobs, size_t count, size_t n, size_t chunk_len, size_t out_len, size_t group_bytes,
                               kzg_recover_batch_info_t* out);

/* ---- G2 on the device: SRS handle, MSM, length commitment and length proof ---------------------------------------------------------
 * The published blob header of the protocol is (commitment in G1, length commitment in G2, length proof in G2, length): with N the
 * order of the setup (a power of two), d <= N the claimed length (a power of two) and f_0 .. f_(d-1) the coefficients,
 *     C = sum f_i [tau^i]_1      C2 = sum f_i [tau^i]_2      pi2 = sum f_i [tau^(N-d+i)]_2
 * and (C, C2, pi2, d) is accepted iff e(C, G2) = e(G1, C2) and e([tau^(N-d)]_1, C2) = e(G1, pi2); the second cannot hold for
 * deg f >= d without a power of tau beyond N - 1.  Both G2 elements are multi-scalar multiplications over G2 powers of tau and run on
 * the GPU (csrc/g2msm.hip: bucket method, signed windows, no tables); G2 wire format as above (16 u64, identity = zeros).
 * Every call below is synchronous, uses slot 0's workspace and stream, and returns KZG_ERR_INVALID_ARG while a kzg_*_begin on slot 0
 * is in flight.  All argument checks run on the host before any launch, in the order written; the context stays usable after any
 * error.  Equal inputs give equal bits, on any context. */
typedef struct kzg_g2srs kzg_g2srs;
/* n_points wire points -> a device-resident G2 SRS (128 B per point).  Every point is checked on the device to be on the twist or
 * the identity: the first one that is not -> KZG_ERR_NOT_ON_CURVE with *bad_index = its position (bad_index may be NULL).  The
 * order-r subgroup is NOT checked, as documented for kzg_verify_proof. */
int32_t kzg_g2srs_upload(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n_points, kzg_g2srs** out, uint64_t* bad_index);
/* [tau^(first_power + i)]_2 for i < n_points and a KNOWN tau (tests, custom setups), computed on the device. */
int32_t kzg_g2srs_generate(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n_points, kzg_g2srs** out);
/* points [offset, offset + n) as wire points; a range outside the handle -> KZG_ERR_INVALID_ARG */
int32_t kzg_g2srs_download(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, size_t n, uint64_t* out_g2_mont);
size_t kzg_g2srs_len(const kzg_g2srs* srs);
void kzg_g2srs_free(kzg_g2srs* srs);
/* sum_i scalars[i] bases[i] in G2 (`G2Projective::msm` + into_affine).  n_bases != n_scalars -> KZG_ERR_MSM_LENGTH_MISMATCH; a base
 * off the twist -> KZG_ERR_NOT_ON_CURVE.  n = 0 gives the identity.  out_is_infinity may be NULL. */
int32_t kzg_msm_g2(kzg_ctx* ctx, const uint64_t* bases_g2_mont, size_t n_bases, const uint64_t* scalars_mont, size_t n_scalars,
                   uint64_t out_g2_mont[16], uint8_t* out_is_infinity);
/* the same over srs[offset .. offset + n): offset + n > kzg_g2srs_len -> KZG_ERR_POLY_LENGTH.  _device: scalars already on the device. */
int32_t kzg_msm_g2_srs(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n,
                       uint64_t out_g2_mont[16], uint8_t* out_is_infinity);
int32_t kzg_msm_g2_srs_device(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* d_scalars_mont, size_t n,
                              uint64_t out_g2_mont[16], uint8_t* out_is_infinity);
/* sum f_i [tau^i]_2 from n coefficients: n > kzg_g2srs_len -> KZG_ERR_POLY_LENGTH. */
int32_t kzg_commit_g2_coeff_form(kzg_ctx* ctx, const kzg_g2srs* srs, const uint64_t* coeffs_mont, size_t n,
                                 uint64_t out_g2_mont[16], uint8_t* out_is_infinity);
/* the same from n evaluations on the n-point domain: inverse Fr NTT on the device, then the MSM.  n not a power of two ->
 * KZG_ERR_NOT_POWER_OF_TWO; n > kzg_g2srs_len -> KZG_ERR_SRS_CAPACITY_EXCEEDED (as kzg_commit_eval_form). */
int32_t kzg_commit_g2_eval_form(kzg_ctx* ctx, const kzg_g2srs* srs, const uint64_t* evals_mont, size_t n,
                                uint64_t out_g2_mont[16], uint8_t* out_is_infinity);
/* The blob header of n coefficients with claimed length claimed_len over a setup of order srs_order: one scalar upload, the G1
 * commitment over g1_srs, and the two G2 MSMs over ONE digit pass and sort (bit for bit what kzg_commit_coeff_form,
 * kzg_commit_g2_coeff_form and kzg_msm_g2_srs return one by one).  g2_trailing holds [tau^(trailing_first_power + i)]_2; the proof is
 * the MSM over its points from offset srs_order - claimed_len - trailing_first_power.  Errors, in order: 1. a null pointer ->
 * KZG_ERR_INVALID_ARG; 2. srs_order or claimed_len not a power of two -> KZG_ERR_NOT_POWER_OF_TWO; 3. n > claimed_len or claimed_len >
 * srs_order -> KZG_ERR_INVALID_ARG; 4. that window not inside g2_trailing (srs_order - claimed_len < trailing_first_power, or its end
 * beyond the handle) -> KZG_ERR_SRS_CAPACITY_EXCEEDED; 5. n larger than g1_srs or g2_srs -> KZG_ERR_POLY_LENGTH. */
int32_t kzg_commit_with_length_proof(kzg_ctx* ctx, const kzg_srs* g1_srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing,
                                     uint64_t trailing_first_power, uint64_t srs_order, const uint64_t* coeffs_mont, size_t n,
                                     uint64_t claimed_len, uint64_t out_commitment_xy[8], uint64_t out_length_commitment[16],
                                     uint64_t out_length_proof[16]);
/* ---- many blobs in one call: the batched G2 MSM over SHARED bases ---------------------------------------------------------------------
 * A disperser publishes one header per blob, and every blob of a call uses the same two base windows (g2_srs[0 .. n) and
 * g2_trailing[off .. off + n)).  `count` blobs are therefore ONE bucket problem per GROUP of blobs: one digit pass, one sort and one
 * launch sequence (the sort's launches and six more, whatever the number of blobs and base sets) carry every blob of the group, so the
 * fixed cost of a short G2 MSM is paid once per group (csrc/g2msm.hip, planned in csrc/g2msm_plan.h).  All outputs are affine wire
 * points: row b is bit for bit what the single call returns for blob b.  count = 0 -> KZG_OK, nothing written; n = 0 -> identities
 * (zeros, flags 1).  count has no cap below 2^20: a call works through its groups.  Synchronous, slot 0, as every G2 call. */
/* count scalar sets of n scalars each, set b at scalars + b n 4, all against srs[offset .. offset + n).  Errors, in order: 1. a null
 * ctx, srs or out, null scalars with n and count non-zero, a handle of another device -> KZG_ERR_INVALID_ARG; 2. count > 2^20 ->
 * KZG_ERR_TOO_LARGE, count n 32 overflowing size_t -> KZG_ERR_INVALID_ARG; 3. offset + n > kzg_g2srs_len -> KZG_ERR_POLY_LENGTH.
 * _device: the scalars are already in device memory. */
int32_t kzg_msm_g2_srs_batch(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n, size_t count,
                             uint64_t* out_g2_mont /* count x 16 */, uint8_t* out_is_infinity /* count, may be NULL */);
int32_t kzg_msm_g2_srs_batch_device(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* d_scalars_mont, size_t n, size_t count,
                                    uint64_t* out_g2_mont /* count x 16 */, uint8_t* out_is_infinity /* count, may be NULL */);
/* count blobs of n coefficients each (blob b at coeffs + b n 4), one claimed length: row b of every output = kzg_commit_with_length_proof
 * on blob b, bit for bit.  The scalars are uploaded once; the G1 commitments are what kzg_commit_coeff_form_batch_device returns for
 * them (g1_srs is not const: that path may build the per-bit tables); the two G2 outputs of a group come from one digit pass and one
 * sort, which both base sets share.  Errors, checked on the host before any launch, in this order: 1. a null pointer (coeffs only
 * when n and count are non-zero) or a handle of another device -> KZG_ERR_INVALID_ARG; 2. count > 2^20 -> KZG_ERR_TOO_LARGE, count n 32
 * overflowing size_t -> KZG_ERR_INVALID_ARG; 3. rows 2 to 5 of kzg_commit_with_length_proof. */
int32_t kzg_commit_with_length_proof_batch(kzg_ctx* ctx, kzg_srs* g1_srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing,
                                           uint64_t trailing_first_power, uint64_t srs_order, const uint64_t* coeffs_mont /* count x n x 4 */,
                                           size_t n, size_t count, uint64_t claimed_len, uint64_t* out_commitments_xy /* count x 8 */,
                                           uint64_t* out_length_commitments /* count x 16 */, uint64_t* out_length_proofs /* count x 16 */);
/* The most blobs per group of the batched G2 calls on this context; 0 = the planner's choice (same results whatever the value). */
int32_t kzg_ctx_set_g2_batch_group(kzg_ctx* ctx, uint32_t max_blobs);
/* What a batched G2 call of `count` blobs of n scalars over nb (1 or 2) base sets would do under max_blobs: a pure query (no context,
 * no device; lanes as planned for a 256-CU device).  The plan fields describe a FULL group.  Single and batched calls share one plan:
 * a batched = 0 row (no two blobs fit one launch) is that plan for one blob -- above 2^22 scalars for the blob's first 2^22 -- with
 * both base sets in every launch: 6 launches behind the sort whatever nb, buffers nb times as large.  Errors: out NULL or nb not 1 or
 * 2 -> KZG_ERR_INVALID_ARG; then row 2 of the tables above.  n = 0 or count = 0: no group (all fields 0). */
typedef struct kzg_g2_batch_info {
    uint64_t blobs_per_group;   /* the last group of a call may hold fewer */
    uint64_t groups;
    uint64_t entries;           /* sorted entries of a full group at most: blobs_per_group x W x n */
    uint64_t workspace_bytes;   /* device buffers of a full group, the sort's included */
    uint32_t batched;           /* 0: no two blobs fit one launch, or a blob is above one launch: groups of one */
    uint32_t c, W;              /* window bits and windows: the single call's */
    uint32_t G;                 /* buckets of one base set: blobs_per_group x W x 2^(c-1) */
    uint32_t nl, seg;           /* accumulate lanes per base set, sorted entries per lane at most */
    uint32_t sort_small;        /* 1: the global-atomic sort (fewer than 2^18 entries), 0: the tiled one */
    uint32_t scan1;             /* 1: the one-workgroup scan of the bucket counts, 0: the three-kernel one */
    uint32_t launches;          /* kernel launches and memsets per group */
    uint32_t reserved;
} kzg_g2_batch_info;
int32_t kzg_msm_g2_batch_info(size_t n, uint32_t nb, size_t count, uint32_t max_blobs, kzg_g2_batch_info* out);
/* The two pairing checks of a header (the top of this section), g1_tau_shift_xy = [tau^(N-d)]_1.  Host only: two calls of the pairing check, no random weight.  A
 * failed check is *out_ok = 0 with KZG_OK.  A G1 input off the curve -> KZG_ERR_G1_NOT_ON_CURVE; a G2 input off the twist ->
 * KZG_ERR_G2_TAU_NOT_ON_CURVE.  The subgroup of the G2 inputs is not checked (see kzg_verify_proof). */
int32_t kzg_verify_length_proof(const uint64_t commitment_xy[8], const uint64_t length_commitment[16], const uint64_t length_proof[16],
                                const uint64_t g1_tau_shift_xy[8], int32_t* out_ok);
/* ---- batches of blob headers ------------------------------------------------------------------------------------------------------
 * A validator checks every header (C, C2, pi2, d) of every batch it signs; the two G2 elements come from an untrusted disperser.
 * kzg_verify_length_proof_batch checks `count` headers with ONE product of pairings: with weights r_i and rho (derived from a
 * transcript of all inputs, or supplied), W_g = sum_{i in g} r_i C2_i per claimed length g, Pi = sum r_i pi2_i, U = sum r_i C_i and
 * S = sum_g W_g it accepts iff
 *     e(U, G2) e(-G1, S + [rho]Pi) prod_g e([rho]T_g, W_g) = 1,      T_g = [tau^(N - shift_lens[g])]_1,
 * which is sum r_i [e(C_i, G2) - e(G1, C2_i)] + rho sum r_i [e(T_(d_i), C2_i) - e(G1, pi2_i)] = 0: 2 + (non-empty groups) Miller loops
 * and one final exponentiation whatever the count.  A batch with a bad header passes with probability about 2^-128 over the weights
 * (independent r_i, one rho between the two equations).  On the device: the on-twist test, the order-r subgroup
 * test of both G2 elements (one 63-bit chain per point, csrc/g2_chain.h), the chains [r_i]C2_i and [r_i]pi2_i with their sums
 * (csrc/g2batch.hip) and the G1 MSM for U.  A rejected batch names no header: kzg_verify_length_proof_batch_locate below finds the bad ones. */
/* host only: prod_k e(g1s[k], g2s[k]) == 1 (EIP-197's predicate), any count; identity inputs contribute 1.
 * G1 off the curve -> KZG_ERR_G1_NOT_ON_CURVE, G2 off the twist -> KZG_ERR_G2_TAU_NOT_ON_CURVE (every G1 input is tested first). */
int32_t kzg_pairings_product_verify(const uint64_t* g1s_xy, const uint64_t* g2s, size_t count, int32_t* out_ok);
/* ---- batches of pairing checks on the device (csrc/pairing.hip, csrc/pairing_dev.h, csrc/fq12.h) ----------------------------------
 * n_checks independent instances of the predicate above in ONE launch: check i covers the pairs [pair_offsets[i], pair_offsets[i + 1])
 * of the two arrays (pair_offsets: n_checks + 1 entries, the first 0, never decreasing), and out_ok[i] (n_checks bytes) is exactly what
 * kzg_pairings_product_verify returns for that slice: identity inputs contribute 1, an empty slice gives 1, a check whose Miller loop
 * meets T = +-Q in an addition step (a G2 point outside the order-r subgroup) gives 0.  One check is one lane's work: the optimal-ate
 * Miller loop of its pairs with a shared squaring, one final exponentiation to the host's exponent, the is-one test.  The on-curve
 * tests run on the device.  Errors, decided in this order, the first three before the context is dereferenced:
 *   a null ctx, pair_offsets or (with n_checks > 0) output; offsets that do not start at 0 or that decrease; a null point array with pairs
 *                                                                                   -> KZG_ERR_INVALID_ARG
 *   n_checks > 2^20, more than 64 pairs in one check, more than 2^20 pairs in all  -> KZG_ERR_TOO_LARGE
 *   a G1 point off the curve (every G1 input is tested first)                      -> KZG_ERR_G1_NOT_ON_CURVE
 *   a G2 point off the twist                                                       -> KZG_ERR_G2_TAU_NOT_ON_CURVE
 * the last two with the first such pair in *bad_index (may be NULL).  No output is written on an error.  n_checks = 0 -> KZG_OK.
 * Synchronous; its buffers are its own (no slot is used).  A lone check takes the time of a full wave of 64 (profiles/pairing_device.md):
 * the batch form pays from a few dozen checks on. */
int32_t kzg_pairings_product_verify_batch(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, uint8_t* out_ok,
                                          uint64_t* bad_index);
/* The same call returning the VALUE of every check: out_gt_mont = n_checks x 12 x 4 u64, the final-exponentiated product as the twelve
 * coefficients of Fq[w] / (w^12 - 18 w^6 + 82) (csrc/host_pairing.h's flat order) in Montgomery wire words; all zero for a check with a
 * degenerate addition step (no GT element).  Arguments and errors as above. */
int32_t kzg_pairings_product_gt_batch(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, uint64_t* out_gt_mont,
                                      uint64_t* bad_index);
/* host only: that value for ONE product of `count` pairs, computed as kzg_pairings_product_verify computes its verdict (chunks of Miller
 * loops, one final exponentiation).  The two GT entries are the parity surface of the device pairing: equal bit for bit.  Errors as
 * kzg_pairings_product_verify. */
int32_t kzg_pairings_product_gt(const uint64_t* g1s_xy, const uint64_t* g2s, size_t count, uint64_t* out_gt_mont);
/* Where the located coset verifiers (kzg_verify_multiproof_batch_locate, kzg_verify_multiproof_batch_locate_bytes,
 * kzg_retrieve_blobs_bytes_tolerant) evaluate pairing checks after a failing root check: 0 (default) = the binary search of
 * csrc/host_locate.h on the host, 1 = the equation of EVERY group as one batch on the device (kzg_pairings_product_verify_batch's
 * kernel).  See "pairing checks of a located batch" at kzg_verify_multiproof_batch_locate.  Another mode -> KZG_ERR_INVALID_ARG. */
int32_t kzg_ctx_set_locate_pairings(kzg_ctx* ctx, int32_t mode);
/* n wire points on the device: each the identity, or on the twist AND in the order-r subgroup.  The first that is not ->
 * KZG_ERR_NOT_ON_CURVE with *bad_index (may be NULL).  n = 0 -> KZG_OK; n > 2^28 -> KZG_ERR_TOO_LARGE.  Synchronous, slot 0. */
int32_t kzg_g2_check_subgroup(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n_points, uint64_t* bad_index);
/* host only: the count + 1 weights of a header batch (r_0 .. r_(count-1), rho), each below 2^128, as Fr wire words.  Two levels, item
 * hashes on the host pool, both tags 24 bytes:
 *   d_i  = SHA-256("KZGBN254_HEADERITEM__V1_" || u64be(claimed_len_i) || ark-compressed C_i || g2bytes(C2_i) || g2bytes(pi2_i))
 *   seed = SHA-256("KZGBN254_HEADERBATCH_V1_" || u64be(count) || u64be(n_shifts) || n_shifts x (u64be(len) || ark-compressed shift) || d_0 .. d_(count-1))
 *   r_i  = the first 16 bytes, read big-endian, of SHA-256(seed || u64be(i));  rho = the same with index `count`
 * g2bytes = be32(x.c0) || be32(x.c1) || be32(y.c0) || be32(y.c1) on canonical integers, the identity 128 zero bytes.  Nothing is
 * validated here. */
int32_t kzg_compute_header_batch_weights(const uint64_t* commitments_xy, const uint64_t* length_commitments, const uint64_t* length_proofs,
                                         const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens,
                                         const uint64_t* g1_tau_shifts_xy, size_t n_shifts, uint64_t* out_weights_mont);
/* shift_lens[g]: distinct powers of two, g1_tau_shifts_xy[g] = [tau^(N - shift_lens[g])]_1; header i belongs to the group whose length
 * is claimed_lens[i].  weights_mont = NULL: the weights above; else (count + 1) x 4 u64, any Fr values (the chains run over the bit
 * length of the largest r_i).  Errors, all checked before the equation, in this order:
 *   1. a null pointer with count > 0, n_shifts = 0 with count > 0, n_shifts > 64, a duplicate shift_lens entry -> KZG_ERR_INVALID_ARG;
 *   2. a shift_lens or claimed_lens entry that is not a power of two -> KZG_ERR_NOT_POWER_OF_TWO;
 *   3. a claimed length that is not in shift_lens -> KZG_ERR_INVALID_ARG with *bad_index = i;
 *   4. count > 2^20 -> KZG_ERR_TOO_LARGE;
 *   5. a commitment or a shift off the curve -> KZG_ERR_G1_NOT_ON_CURVE (commitments first; a shift reports its position in the list);
 *   6. a G2 input off the twist -> KZG_ERR_G2_TAU_NOT_ON_CURVE;
 *   7. a G2 input outside the order-r subgroup -> KZG_ERR_NOT_ON_CURVE.
 * 5-7 set *bad_index (may be NULL) to the header's index, the smallest one, C2 tested in front of pi2.  count = 0 -> *out_ok = 1.  A
 * failed equation is *out_ok = 0 with KZG_OK.  Identity C, C2 and pi2 (the zero polynomial) form a valid header.  Synchronous, slot
 * 0 (KZG_ERR_INVALID_ARG while a _begin on slot 0 is in flight); the context is usable after any error.  KZG_VB_TRACE=1 prints the
 * phase times on stderr. */
int32_t kzg_verify_length_proof_batch(kzg_ctx* ctx, const uint64_t* commitments_xy, const uint64_t* length_commitments,
                                      const uint64_t* length_proofs, const uint64_t* claimed_lens, size_t count,
                                      const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                                      const uint64_t* weights_mont /* NULL: derived */, int32_t* out_ok, uint64_t* bad_index);
/* Locating the bad headers of a rejected batch.  The equation above is linear in the set of headers, so for ANY partition of the headers
 * into n_groups groups (group_indices[i] < n_groups is header i's group; a group may be empty) the device produces, in one pass over the
 * batch, the components of every group's own equation, with the weights of the batch entry (weights_mont, or derived when NULL):
 *     U_g     = sum_{i in g} r_i C_i                              (G1)
 *     W_{g,s} = sum_{i in g, d_i = shift_lens[s]} r_i C2_i        (G2, s < n_shifts)
 *     Pi_g    = sum_{i in g} r_i pi2_i                            (G2)
 * Group g is good iff  e(U_g, G2) e(-G1, sum_s W_{g,s} + [rho]Pi_g) prod_s e([rho]T_s, W_{g,s}) = 1.  Summed over all groups the
 * components are those of the batch entry, so the verdict on the sum of all groups is that entry's verdict for the same inputs and
 * weights; the equation of any union of groups is the same predicate on the component-wise sums.
 *
 * kzg_header_group_sums: the inputs of the batch entry, the partition, and the outputs out_u_xy (n_groups x 8 u64, affine G1 wire points)
 * with out_u_is_infinity (n_groups bytes), out_w_g2 (n_groups x n_shifts x 16 u64, row g n_shifts + s = W_{g,s}) and out_pi_g2 (n_groups
 * x 16 u64): affine wire points, the G2 identity all zeros; an empty group, and a length no header of a group claims, give identities.
 * Equal inputs give equal bits, whatever the order of the headers inside a group and whatever the launch geometry.  On the device: the
 * G2 points lie one per lane in the sorted order of a composite key (g n_shifts + s for C2_i, n_groups n_shifts + g for pi2_i; the
 * stable counting sort of csrc/host_locate.h, a permutation), every lane runs its chain [r_i]P, a segmented scan over the wave and one
 * wave per segment leave the sums (csrc/g2batch.hip); U_g takes the GLV multiplication and the segmented scan of the coset entries
 * (csrc/multilocate.hip), keyed by group.
 * Errors: rows 1-7 of the batch entry's table in its order (a null group_indices with count > 0, or a null output with n_groups > 0,
 * counts as a null pointer under row 1), with two rows behind row 4, before any curve check or allocation:
 *   4a. a group index >= n_groups, or n_groups = 0 with count > 0 -> KZG_ERR_INVALID_ARG;
 *   4b. n_groups * (n_shifts + 1) > 2^28 -> KZG_ERR_TOO_LARGE.
 * count = 0 -> identities everywhere, no device work.  Synchronous, slot 0 (KZG_ERR_INVALID_ARG while a _begin on slot 0 is in
 * flight); the context is usable after any error. */
int32_t kzg_header_group_sums(kzg_ctx* ctx, const uint64_t* commitments_xy, const uint64_t* length_commitments,
                              const uint64_t* length_proofs, const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens,
                              const uint64_t* g1_tau_shifts_xy, size_t n_shifts, const uint64_t* weights_mont /* NULL: derived */,
                              const uint64_t* group_indices, size_t n_groups, uint64_t* out_u_xy, uint8_t* out_u_is_infinity,
                              uint64_t* out_w_g2, uint64_t* out_pi_g2, uint64_t* bad_index);
/* The group sums above, then a search on the host (the one of kzg_verify_multiproof_batch_locate): prefix sums of the groups' components
 * in group order make the components of any range of groups a difference of two prefixes; the root is tested first; a range that holds
 * marks all its groups good; a failing range of one group marks it bad; any other failing range is halved and its left half tested (if
 * that holds, the right half fails without a test).  Each test is one product of pairings on the host pool, 3 + (lengths present in
 * the batch) Miller loops with rho on the G1 side (e(-[rho]G1, Pi) for e(-G1, [rho]Pi); [rho]G1 and [rho]T_s are computed once per
 * call), and no GPU work: at most 1 + 2 b ceil(log2 n_groups) checks for b bad groups, exactly one for a good batch.  out_group_ok:
 * n_groups bytes, 1 = good; *out_bad_groups = the number of bad groups; *out_pairing_checks (may be NULL) = the checks made.  KZG_OK
 * with *out_bad_groups = 0 is the accept of the batch entry.  The host work in front of the search is linear in n_groups x (2 + lengths
 * present): with one group per header and very large counts it outweighs the device pass, so group coarsely first (profiles/header_locate.md).
 * Soundness: a range that holds could in principle hide bad groups that cancel; with weights derived from the transcript over ALL
 * inputs (weights_mont = NULL, or kzg_compute_header_batch_weights) that has negligible probability, with weights of the caller's own
 * choosing there is no such guarantee.
 * This entry always pays for the group sums: a caller who expects good batches calls the batch entry first and this one only after a
 * reject.  count = 0 -> every group good, no device work, no pairing check.  Errors: those of kzg_header_group_sums in its order
 * (a null out_bad_groups, or a null out_group_ok with n_groups > 0, under row 1).  Synchronous, slot 0.  KZG_VB_TRACE=1 prints the
 * phases on stderr: shared prefix, G2 group sums, G1 group sums, host sums, search with its number of checks. */
int32_t kzg_verify_length_proof_batch_locate(kzg_ctx* ctx, const uint64_t* commitments_xy, const uint64_t* length_commitments,
                                             const uint64_t* length_proofs, const uint64_t* claimed_lens, size_t count,
                                             const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                                             const uint64_t* weights_mont /* NULL: derived */, const uint64_t* group_indices,
                                             size_t n_groups, uint8_t* out_group_ok, size_t* out_bad_groups,
                                             size_t* out_pairing_checks /* may be NULL */, uint64_t* bad_index);
/* n_points gnark-compressed G2 points (64 bytes each: X.A1 || X.A0 big-endian, top two bits of the first byte 0b10 = the smaller y,
 * 0b11 = the larger; the format of the reference's g2.point.powerOf2) -> wire points, on the library's host thread pool.  Flag bits
 * not 0b10 / 0b11 or a coordinate not below the modulus -> KZG_ERR_DESERIALIZE; no point of that x on the twist, a point outside the
 * order-r subgroup, or the generator itself -> KZG_ERR_NOT_ON_CURVE; *bad_index = the first such point (may be NULL).  Host only. */
int32_t kzg_g2_decompress_be(const uint8_t* bytes, size_t n_points, uint64_t* out_g2_mont, uint64_t* bad_index);
/* The same format decoded ON THE DEVICE (csrc/g2_decode.h, csrc/g2decode.hip: one lane per point, the square root in Fq2 with two
 * exponentiations, the 63-bit subgroup chain of csrc/g2_chain.h): the host decoder above costs about a millisecond per point and thread.
 * The bytes are staged in chunks through pinned memory the context already holds.  Per point, in this order: 1. flag bits not 0b10 /
 * 0b11 -> KZG_ERR_DESERIALIZE; 2. a coordinate not below the modulus -> KZG_ERR_DESERIALIZE; 3. no point of that x on the twist ->
 * KZG_ERR_NOT_ON_CURVE; 4. with KZG_G2_CHECK_SUBGROUP: not in the order-r subgroup -> KZG_ERR_NOT_ON_CURVE; 5. with
 * KZG_G2_REJECT_GENERATOR: the generator itself -> KZG_ERR_NOT_ON_CURVE.  The status is that of the SMALLEST bad index, which goes to
 * *bad_index (may be NULL).  Synchronous, slot 0. */
#define KZG_G2_CHECK_SUBGROUP   1u
#define KZG_G2_REJECT_GENERATOR 2u
/* n_points compressed points (host bytes) -> wire points (host).  flags = 3: status, *bad_index and bits are those of
 * kzg_g2_decompress_be on the same bytes; flags = 0: on the twist only.  Errors, in order: 1. a null pointer with n_points > 0, or a
 * flag bit other than the two above -> KZG_ERR_INVALID_ARG; 2. n_points > 2^28 -> KZG_ERR_TOO_LARGE (nothing is allocated); 3. a
 * kzg_*_begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 4. the points, as above: then out_g2_mont is not written.  n_points = 0 ->
 * KZG_OK. */
int32_t kzg_g2_decompress_be_device(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, uint32_t flags, uint64_t* out_g2_mont,
                                    uint64_t* bad_index);
/* The same into a device-resident G2 SRS, without a wire round trip.  Every point is subgroup-checked; the generator is accepted (a
 * file of powers of tau starts with [tau^0]_2).  Errors as above (1. also: out NULL); on any error *out = NULL. */
int32_t kzg_g2srs_load_compressed_be(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_g2srs** out, uint64_t* bad_index);

/* ---- coset items in their serialized form (csrc/g1_decode.h, csrc/cosetbytes.hip, csrc/host_coset_bytes.h) ---------------------------
 * What a sampler or validator receives off the wire: a commitment or proof is a 32-byte gnark-compressed G1 point (x big-endian, the
 * top two bits of byte 0: 0b01 = the identity, written 0x40 || 31 zero bytes; 0b10 / 0b11 = the smaller / larger y by
 * lexicographically_largest), a value is a 32-byte big-endian scalar.  Decoding is STRICT, per element in this order: 1. flag bits
 * 0b00 (gnark's uncompressed marker), or 0b01 with any other bit set -> KZG_ERR_DESERIALIZE; 2. x >= p -> KZG_ERR_DESERIALIZE (the SRS
 * loader kzg_srs_load_compressed_be reduces such an x mod p as the reference does; here one byte string names one point, so that the
 * transcript over the bytes equals the transcript over the decoded points); 3. x^3 + 3 not a square -> KZG_ERR_NOT_ON_CURVE; a value
 * >= r -> KZG_ERR_DESERIALIZE.  G1 has cofactor 1: a point on the curve is in the group.  The status of an array is that of its
 * SMALLEST bad index, whatever the launch geometry.  Host bytes are staged in chunks through pinned memory the context already holds.
 * The device entries are synchronous on slot 0 (KZG_ERR_INVALID_ARG while a kzg_*_begin is in flight on it); every argument check runs
 * on the host before any launch and the context stays usable after any error.
 *
 * kzg_g1_decompress_be_device: n_points points -> wire points (n_points x 8 u64; the identity as the all-zero wire point) and,
 * when out_is_infinity is not NULL, one identity byte per point.  Errors, in order: 1. a null ctx, or null bytes / out_xy_mont with
 * n_points > 0 -> KZG_ERR_INVALID_ARG; 2. n_points > 2^28 -> KZG_ERR_TOO_LARGE; 3. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG;
 * 4. the points, as above, *bad_index (may be NULL) = the smallest bad index: then the outputs are not written.  n_points = 0 -> KZG_OK. */
int32_t kzg_g1_decompress_be_device(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, uint64_t* out_xy_mont,
                                    uint8_t* out_is_infinity /* may be NULL */, uint64_t* bad_index);
/* A batch of items -> the wire words kzg_verify_multiproof_batch_locate, kzg_coset_group_sums and kzg_recover_from_cosets take: ys_be
 * count x chunk_len x 32 bytes -> out_ys_mont count x chunk_len x 4 u64; proofs_be count x 32 bytes -> out_proofs_xy_mont count x 8
 * u64.  Either input / output pair may be NULL together (recovery decodes values only).  Errors, in order: 1. a null ctx, one pointer
 * of a pair NULL and the other not, both pairs NULL with count > 0, chunk_len = 0 with values -> KZG_ERR_INVALID_ARG; 2. count *
 * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE; 3. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 4. a bad proof: *bad_array = 1,
 * *bad_index = its item; 5. a bad value: *bad_array = 2, *bad_index = its ITEM (both may be NULL).  On an error of 4 / 5 the outputs
 * are not written.  count = 0 -> KZG_OK. */
int32_t kzg_coset_items_decode_be(kzg_ctx* ctx, const uint8_t* ys_be, const uint8_t* proofs_be, size_t count, size_t chunk_len,
                                  uint64_t* out_ys_mont, uint64_t* out_proofs_xy_mont, uint64_t* bad_index, int32_t* bad_array);
/* The disperser's half, host only (the library's host pool): Montgomery words -> canonical big-endian values, wire points ->
 * compressed points with their sign bit, the all-zero wire point -> 0x40 || zeros.  Pairs may be NULL together as above.  The inputs
 * are trusted (a point is not checked to be on the curve).  Errors: the pointer / chunk_len rules of kzg_coset_items_decode_be ->
 * KZG_ERR_INVALID_ARG; count * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE; a value or coordinate not below its modulus ->
 * KZG_ERR_INVALID_ARG (the outputs are then unspecified). */
int32_t kzg_coset_items_encode_be(const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t count, size_t chunk_len,
                                  uint8_t* out_ys_be, uint8_t* out_proofs_be);
/* The weights of kzg_compute_multiproof_r_powers, bit for bit, from the serialized form of the same items, for every input whose
 * bytes decode.  Host only.  The item message is assembled from the bytes: be32(ys_i[j]) is the value's bytes as they are, the
 * ark-compressed point is the gnark bytes reversed with the flag bits remapped (0b10 -> 0, 0b11 -> 0x80, 0b01 -> 0x40); no field
 * multiplication occurs before the final mod r.  Bytes that do not decode are hashed as given (flag 0b00 -> 0xC0), not validated, like
 * the existing entry.  Arguments and errors as kzg_compute_multiproof_r_powers. */
int32_t kzg_compute_multiproof_r_powers_bytes(const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices,
                                              const uint64_t* coset_indices, const uint8_t* ys_be, const uint8_t* proofs_be, size_t count,
                                              size_t n, size_t chunk_len, uint64_t* out_r_powers_mont);
/* kzg_verify_multiproof_batch with the decode inside the call: the verdict of that entry on the decoded inputs, and the same weights
 * bit for bit (r_powers_mont = NULL derives them; out_r_powers_mont, may be NULL, receives the count weights used).  Values go up once
 * as bytes and are decoded where the interpolation kernel reads them; proofs and commitments go up as 32 bytes each and are decoded
 * into the bases of the batched MSMs (the decode kernel writes the second copy of the proofs for the r_i w^(k_i l) combination); nothing
 * decoded returns to the host.  Derived weights read the bytes: on the host pool beside the decode kernels, or -- inside the automatic
 * envelope, or when kzg_ctx_set_transcript_device forces it -- on the device, hashing the uploaded bytes.  Device memory: the value
 * bytes (count x chunk_len x 32) on top of what the decoded entry uses.
 * Errors, in this order: 1. those of kzg_verify_multiproof_batch up to and including the index checks and count * chunk_len > 2^28;
 * a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 2. a bad commitment (*bad_array = 0); 3. a bad proof (*bad_array = 1); 4. a bad
 * value (*bad_array = 2), each with the status of the decode rules above and *bad_index = the commitment / item (both may be NULL);
 * 5. g2_tau_l_mont off the twist -> KZG_ERR_G2_TAU_NOT_ON_CURVE.  count = 0 -> *out_ok = 1.  KZG_VB_TRACE=1 prints the phase times,
 * `decode` among them, on stderr. */
int32_t kzg_verify_multiproof_batch_bytes(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* commitments_be, size_t n_commitments,
                                          const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint8_t* ys_be,
                                          const uint8_t* proofs_be, size_t count, size_t n, size_t chunk_len,
                                          const uint64_t* r_powers_mont /* NULL: derived */, const uint64_t* g2_tau_l_mont, int32_t* out_ok,
                                          uint64_t* out_r_powers_mont /* may be NULL */, uint64_t* bad_index, int32_t* bad_array);
/* ---- the retriever's half in serialized form (csrc/recover.hip, csrc/host_recover.h) --------------------------------------------------
 * kzg_recover_from_cosets_batch with the codec inside the call: big-endian values in, big-endian rows out.  For every input whose
 * values decode, row b of out_polys_be is kzg_coset_items_encode_be of row b of kzg_recover_from_cosets_batch on the output of
 * kzg_coset_items_decode_be, byte for byte, and out_consistent[b] is that call's flag.  The values go up once, as bytes, and are
 * decoded where the first kernel loads them; the rows are encoded where the last kernel stores them; no word form crosses the bus.
 * Errors, in this order: 1 .. 8. the table of kzg_recover_from_cosets_batch, unchanged; 9. blobs * count * chunk_len > 2^28 ->
 * KZG_ERR_TOO_LARGE; 10. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 11. a value >= r -> KZG_ERR_DESERIALIZE, *bad_index (may
 * be NULL) = the ITEM b * count + i of the smallest bad value.  The blobs are worked through in the groups of kzg_recover_batch_info,
 * in order, and the call ends at the first group that holds a bad value: rows of that group and of earlier ones may already have been
 * written, flags of earlier ones only.  The context stays usable after any error. */
int32_t kzg_recover_from_cosets_batch_bytes(kzg_ctx* ctx, const uint8_t* ys_be /* blobs x count x chunk_len x 32 */,
                                            const uint64_t* coset_indices /* index_rows x count */, size_t index_rows, size_t blobs,
                                            size_t count, size_t n, size_t chunk_len, size_t degree_bound, int32_t eval_form,
                                            size_t out_len /* 0 = n */, uint8_t* out_polys_be /* blobs x out_len x 32 */,
                                            int32_t* out_consistent /* blobs, may be NULL */, uint64_t* bad_index /* may be NULL */);
/* The retriever's call: verify the chunks of `blobs` blobs against their commitments and, if the batch is accepted, recover the blobs.
 * *out_ok, the weights (r_powers_mont = NULL derives them: the same bits) and every decode refusal (*bad_array 0 / 1 / 2, *bad_index)
 * are those of kzg_verify_multiproof_batch_bytes on the blobs x count items with n_commitments = blobs, commitment_indices[i] = i /
 * count and the coset indices flattened (a single row repeated per blob).  With *out_ok = 1 the outputs are those of
 * kzg_recover_from_cosets_batch_bytes on the same values.  With *out_ok = 0 the status is KZG_OK, no recovery kernel runs and
 * out_polys_be / out_consistent are not written: go to kzg_verify_multiproof_batch_locate.  The values are uploaded once; the recovery
 * reads the bytes where the verifier's front end left them on the device.  Device memory: what both halves use today, held side by side.
 * Errors, in this order, the first two groups on the host before anything is launched: 1. rows 1 .. 9 of
 * kzg_recover_from_cosets_batch_bytes (its pointers: ctx, ys_be, coset_indices, out_polys_be); 2. the host checks of
 * kzg_verify_multiproof_batch_bytes (its pointers: srs, commitments_be, proofs_be, out_ok, g2_tau_l_mont when chunk_len != 1; the SRS;
 * chunk_len > the SRS), a _begin in flight on slot 0; 3. that entry's device-side refusals in its order (commitment, proof, value, then
 * g2_tau_l_mont off the twist).  KZG_VB_TRACE=1 prints the phase times, `recover` among them, on stderr. */
int32_t kzg_retrieve_blobs_bytes(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* commitments_be /* blobs x 32 */,
                                 const uint64_t* coset_indices, size_t index_rows, const uint8_t* ys_be,
                                 const uint8_t* proofs_be /* blobs x count x 32 */, size_t blobs, size_t count, size_t n, size_t chunk_len,
                                 size_t degree_bound, int32_t eval_form, size_t out_len, const uint64_t* r_powers_mont /* NULL: derived */,
                                 const uint64_t* g2_tau_l_mont, int32_t* out_ok, uint8_t* out_polys_be, int32_t* out_consistent,
                                 uint64_t* bad_index, int32_t* bad_array);
/* kzg_verify_multiproof_batch_locate on serialized items: the front end of kzg_verify_multiproof_batch_bytes, then the group sums and the
 * search of the decoded entry over what that front end left on the device.  For every input whose bytes decode, out_group_ok,
 * *out_bad_groups and *out_pairing_checks are those of kzg_verify_multiproof_batch_locate on the output of kzg_coset_items_decode_be
 * (with the commitments decoded), and the weights are the same bit for bit (r_powers_mont = NULL derives them; out_r_powers_mont, may be
 * NULL, receives the count weights used).  Values, proofs and commitments go up once, as bytes; nothing decoded returns to the host.
 * Errors, in this order: 1. the host checks of kzg_verify_multiproof_batch_locate, in its order (null pointers: those of the bytes entry
 * with out_bad_groups, out_group_ok when n_groups > 0 and group_indices when count > 0; ...; a group index >= n_groups; count *
 * chunk_len > 2^28; n_groups > 2^28); 2. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 3. the decode refusals exactly as
 * kzg_verify_multiproof_batch_bytes reports them: a bad commitment (*bad_array = 0), a bad proof (1), a bad value (2), *bad_index, the
 * status of the smallest bad index; 4. g2_tau_l_mont off the twist -> KZG_ERR_G2_TAU_NOT_ON_CURVE.  count = 0: every group good, no
 * device work, no pairing check.  KZG_VB_TRACE=1 prints the phase times on stderr. */
int32_t kzg_verify_multiproof_batch_locate_bytes(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* commitments_be, size_t n_commitments,
                                                 const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint8_t* ys_be,
                                                 const uint8_t* proofs_be, size_t count, size_t n, size_t chunk_len,
                                                 const uint64_t* r_powers_mont /* NULL: derived */, const uint64_t* g2_tau_l_mont,
                                                 const uint64_t* group_indices, size_t n_groups, uint8_t* out_group_ok,
                                                 size_t* out_bad_groups, size_t* out_pairing_checks /* may be NULL */,
                                                 uint64_t* out_r_powers_mont /* may be NULL */, uint64_t* bad_index, int32_t* bad_array);
/* The retriever's call that survives bad chunks.  A retriever holds `count` chunks per blob, more than it needs, from operators it does
 * not trust: this call names the bad chunks and recovers every blob from its first use_count good ones, in item order.  Items and
 * arguments as kzg_retrieve_blobs_bytes; out_ok is replaced by
 *   out_item_status[b * count + j]   0 good; 1 decodes but fails its equation; 2 proof bytes not canonical (flag bits, x >= p); 3 the
 *                                    proof's x has no point on the curve; 4 a value >= r.  The smallest of 2 / 3 / 4 that applies
 *                                    wins: a proof is reported before a value, as in the other entries;
 *   out_blob_status[b]               0 recovered; 1 fewer than use_count good items: row b of out_polys_be is zero bytes and
 *                                    out_consistent[b] = 0;
 *   *out_bad_items, *out_unrecovered the number of items of status != 0 and of blobs of status 1;
 *   *out_pairing_checks              (may be NULL) the pairing checks spent.
 * A commitment that does not decode stays a call error (*bad_array = 0): it is the retriever's own input.
 * Weights: r_powers_mont = NULL derives those of kzg_compute_multiproof_r_powers_bytes on the bytes AS GIVEN (both transcript paths hash
 * bytes and decode nothing, so a refusal changes no weight); then every refused item (status 2 / 3 / 4) enters every sum with weight 0
 * -- a small kernel zeroes them on the device -- and every other item keeps its weight.  out_r_powers_mont (may be NULL) receives the
 * blobs x count weights used: those bits, zero at every refused item.  The status arrays, the counts and the weights are written behind
 * the last step that can fail: an error leaves them as the caller handed them in.  The context's lock is held for the whole call, the
 * host-side pairing checks included (the located pass and the recovery read what the front end left on the device).
 * Equation: the batch equation runs once.  If it holds, every non-refused item is good and *out_pairing_checks = 1.  If it fails, the bad
 * items are located on what the front end left on the device -- no byte crosses the bus again, no weight is derived again, the per-item
 * rows r_i w^(-k_i t) IFFT_l(ys_i)_t are computed once -- in two levels with the search of kzg_verify_multiproof_batch_locate: groups =
 * blobs, then groups = the single non-refused items of the bad blobs only (segment sums, group MSMs and point sums over that subset).
 * *out_pairing_checks <= 1 + (1 + 2 B ceil(log2 blobs)) + (1 + 2 b ceil(log2 I)) for B bad blobs, their I items and b bad items.
 * Recovery: rows and flags of a recovered blob are byte for byte those of kzg_recover_from_cosets_batch_bytes on its chosen chunks (one
 * index row per blob, the same degree_bound, eval_form and out_len); the value bytes are read where the verifier left them.  With
 * use_count = count and nothing bad, rows and flags are those of kzg_retrieve_blobs_bytes.  All of the above returns KZG_OK.
 * Errors, in this order, 1 and 2 on the host before anything is launched: 1. the recovery's table: a null ctx, ys_be, coset_indices,
 * out_polys_be, out_item_status, out_blob_status, out_bad_items or out_unrecovered, or blobs = 0 -> KZG_ERR_INVALID_ARG; index_rows not
 * 1 or blobs -> KZG_ERR_INVALID_ARG; n not a power of two -> KZG_ERR_NOT_POWER_OF_TWO; n > 2^24 -> KZG_ERR_DOMAIN; n = 1, chunk_len not
 * a power of two or > n / 2, count = 0 or > n / chunk_len, use_count = 0 or > count -> KZG_ERR_INVALID_ARG; a coset index >= n /
 * chunk_len or twice in one row -> KZG_ERR_INVALID_ARG; degree_bound > use_count * chunk_len -> KZG_ERR_INVALID_ARG; out_len (evaluations:
 * not n; coefficients: below the bound or above n) -> KZG_ERR_INVALID_ARG; (n / chunk_len) * (n / chunk_len - use_count) > 2^32 ->
 * KZG_ERR_TOO_LARGE; blobs * n * 32 overflows -> KZG_ERR_INVALID_ARG; blobs * count * chunk_len > 2^28 -> KZG_ERR_TOO_LARGE; 2. the host
 * checks of kzg_verify_multiproof_batch_bytes (srs, commitments_be, proofs_be, g2_tau_l_mont when chunk_len != 1; the SRS; chunk_len >
 * the SRS); 3. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 4. a bad commitment, *bad_array = 0, *bad_index = the blob;
 * 5. g2_tau_l_mont off the twist.  KZG_VB_TRACE=1 prints the phase times on stderr. */
int32_t kzg_retrieve_blobs_bytes_tolerant(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* commitments_be /* blobs x 32 */,
                                          const uint64_t* coset_indices, size_t index_rows, const uint8_t* ys_be,
                                          const uint8_t* proofs_be /* blobs x count x 32 */, size_t blobs, size_t count, size_t use_count,
                                          size_t n, size_t chunk_len, size_t degree_bound, int32_t eval_form, size_t out_len,
                                          const uint64_t* r_powers_mont /* NULL: derived */, const uint64_t* g2_tau_l_mont,
                                          uint8_t* out_item_status /* blobs x count */, uint8_t* out_blob_status /* blobs */,
                                          size_t* out_bad_items, size_t* out_unrecovered, size_t* out_pairing_checks /* may be NULL */,
                                          uint8_t* out_polys_be, int32_t* out_consistent /* may be NULL */,
                                          uint64_t* out_r_powers_mont /* may be NULL */, uint64_t* bad_index, int32_t* bad_array);

/* ---- blob headers in their serialized form (csrc/headerbytes.hip, csrc/header_item_stream.h, csrc/host_header_bytes.h) ---------------
 * What a validator receives off the wire, per header (C, C2, pi2, d): the commitment as 32 bytes in the G1 format above (identity 0x40
 * || 31 zeros, strict); the length commitment and the length proof as 64 bytes each in the G2 format of kzg_g2_decompress_be (X.A1 ||
 * X.A0 big-endian, 0b10 / 0b11 = the smaller / larger y) EXTENDED BY THE IDENTITY, 0b01 with every other bit zero, written 0x40 || 63
 * zero bytes (the header of the zero polynomial is valid); the claimed lengths stay a uint64_t array.  Decoding a G2 element, in this
 * order: 1. flag bits 0b00, or 0b01 with any other bit set -> KZG_ERR_DESERIALIZE; 2. a coordinate >= p -> KZG_ERR_DESERIALIZE; 3. no
 * point of that x on the twist -> KZG_ERR_NOT_ON_CURVE; 4. a point outside the order-r subgroup -> KZG_ERR_NOT_ON_CURVE.  The generator
 * is a valid element (f = 1).  kzg_g2_decompress_be_device keeps its own rule: it has no identity.  One byte string names one point, so
 * the header transcript over the decoded points is a function of the bytes.
 *
 * kzg_header_items_encode_be: the disperser's half, host only (the library's host pool): wire points -> the three byte arrays (32, 64,
 * 64 bytes per header); the all-zero wire point encodes as the identity.  The inputs are trusted (no curve or subgroup check).  Each
 * input / output pair may be NULL together.  Errors: one pointer of a pair NULL and the other not, or all pairs NULL with count > 0 ->
 * KZG_ERR_INVALID_ARG; count > 2^20 -> KZG_ERR_TOO_LARGE; a coordinate not below p -> KZG_ERR_INVALID_ARG (the outputs are then
 * unspecified). */
int32_t kzg_header_items_encode_be(const uint64_t* commitments_xy, const uint64_t* length_commitments, const uint64_t* length_proofs,
                                   size_t count, uint8_t* out_commitments_be, uint8_t* out_length_commitments_be,
                                   uint8_t* out_length_proofs_be);
/* The byte arrays -> the wire points the decoded header entries take, on the device: commitments count x 8 u64, G2 elements count x 16
 * u64 each, an identity all zeros.  Every G2 element is subgroup-checked.  Errors, in order: 1. a null ctx, or any null array with
 * count > 0 -> KZG_ERR_INVALID_ARG; 2. count > 2^20 -> KZG_ERR_TOO_LARGE; 3. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 4. a
 * bad commitment: *bad_array = 0; 5. a bad G2 element: *bad_array = 1 (length commitment) or 2 (length proof), the smallest header
 * that has one, its length commitment in front of its length proof; *bad_index = the header (both may be NULL).  On an error of 4 / 5
 * the outputs are not written.  count = 0 -> KZG_OK.  Synchronous, slot 0. */
int32_t kzg_header_items_decode_be(kzg_ctx* ctx, const uint8_t* commitments_be, const uint8_t* length_commitments_be,
                                   const uint8_t* length_proofs_be, size_t count, uint64_t* out_commitments_xy,
                                   uint64_t* out_length_commitments, uint64_t* out_length_proofs, uint64_t* bad_index, int32_t* bad_array);
/* kzg_verify_length_proof_batch with the decode inside the call: for every input that decodes, *out_ok is that entry's on the output
 * of kzg_header_items_decode_be, and the weights are the same bit for bit (weights_mont = NULL derives them; out_weights_mont, may be
 * NULL, receives the count + 1 weights used).  One pass on the device decodes the G2 elements where the chains read them and runs the
 * order-r subgroup test there, the ONE 63-bit chain an element gets; the commitments are decoded into the bases of the G1 MSM; nothing
 * decoded returns to the host.  Derived weights: the item digests are hashed on the device, one lane per header, from the commitment's
 * bytes and the decoded G2 points (32 bytes per header come down); the batch hash, the count + 1 weight hashes and the bit length of
 * the largest weight stay on the host.  With supplied weights no digest kernel runs.
 * Errors, in this order: 1. rows 1-4 of kzg_verify_length_proof_batch's table, on the host before any launch; 2. a _begin in flight on
 * slot 0 -> KZG_ERR_INVALID_ARG; 3. a shift off the curve -> KZG_ERR_G1_NOT_ON_CURVE, *bad_array = 3, *bad_index = its position in the
 * list; 4. a bad commitment: *bad_array = 0; 5. a bad G2 element: *bad_array = 1 / 2 as for kzg_header_items_decode_be; 4 and 5 with the
 * status of the decode rules above and *bad_index = the header (both may be NULL).  count = 0 -> *out_ok = 1, no device work.  The
 * context is usable after any error.  KZG_VB_TRACE=1 prints the phase times, `decode` and `digests` among them, on stderr. */
int32_t kzg_verify_length_proof_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments_be, const uint8_t* length_commitments_be,
                                            const uint8_t* length_proofs_be, const uint64_t* claimed_lens, size_t count,
                                            const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                                            const uint64_t* weights_mont /* NULL: derived */, int32_t* out_ok,
                                            uint64_t* out_weights_mont /* may be NULL */, uint64_t* bad_index, int32_t* bad_array);
/* kzg_verify_length_proof_batch_locate on serialized headers: the same prefix as the entry above, then the group sums and the search of
 * the decoded entry; out_group_ok, *out_bad_groups and *out_pairing_checks are that entry's on the output of
 * kzg_header_items_decode_be.  The commitments are decoded where the G1 group sums read them: nothing decoded returns to the host.
 * Errors: as above, with rows 4a / 4b of the grouped entries behind row 4. */
int32_t kzg_verify_length_proof_batch_locate_bytes(kzg_ctx* ctx, const uint8_t* commitments_be, const uint8_t* length_commitments_be,
                                                   const uint8_t* length_proofs_be, const uint64_t* claimed_lens, size_t count,
                                                   const uint64_t* shift_lens, const uint64_t* g1_tau_shifts_xy, size_t n_shifts,
                                                   const uint64_t* weights_mont /* NULL: derived */, const uint64_t* group_indices,
                                                   size_t n_groups, uint8_t* out_group_ok, size_t* out_bad_groups,
                                                   size_t* out_pairing_checks /* may be NULL */, uint64_t* bad_index, int32_t* bad_array);

/* ---- the disperser's half in serialized form (csrc/multiproof.hip, csrc/g1_decode.h) ---------------------------------------------------
 * kzg_encode_cosets_batch with the codec inside the call: blobs of 32-byte big-endian field elements in, serialized chunks out.  For
 * every input whose bytes decode (kzg_coset_items_decode_be's rule for a value: canonical, a value >= r is refused, not reduced),
 * out_ys_be and out_proofs_be are kzg_coset_items_encode_be of kzg_encode_cosets_batch on the decoded blobs, byte for byte, and
 * out_commitments_be is the compressed kzg_commit_coeff_form_batch of the blobs' coefficients (with eval_form = 1 that is also the
 * compressed kzg_commit_eval_form_batch: a point has one affine form; it is computed from the coefficients the call holds after its
 * inverse transform, no Lagrange basis is built).  Each output may be NULL (it is then not computed), not all three.
 * The groups, their plans and the byte budget are kzg_encode_cosets_batch's (kzg_encode_cosets_batch_info,
 * kzg_ctx_set_encode_group_bytes), a shape that runs as groups of one included.  Per group the blobs go up once, as bytes, into the
 * buffer the words would have gone to, and are decoded where the group's first kernel loads them; the value rows are encoded where
 * the gather kernel stores them (32 bytes a value), the proofs are compressed by the affine conversion behind FK20 (32 bytes a proof,
 * the identity 0x40 || zeros: no flag array); the commitments are the batched G1 MSM over the resident coefficients, one wire point a
 * blob, compressed on the host.  Device memory: that of kzg_encode_cosets_batch plus 64 bytes.
 * Errors, in this order, 1 - 3 on the host before anything is launched: 1. rows 1 - 7 of kzg_encode_cosets_batch with this entry's
 * pointers (ctx, srs, blobs_be; all three outputs NULL -> KZG_ERR_INVALID_ARG); 2. count * poly_len > 2^28 -> KZG_ERR_TOO_LARGE; 3. a
 * _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 4. a value >= r -> KZG_ERR_DESERIALIZE, *bad_index (may be NULL) = b * poly_len + i
 * of the smallest bad value of the first group that holds one.  The groups run in order and the call ends at that group, before any
 * of its outputs is written; outputs of earlier groups have been.  The context stays usable after any error. */
int32_t kzg_encode_cosets_batch_bytes(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* blobs_be /* count x d x 32 */, size_t count,
                                      size_t poly_len /* d */, int32_t eval_form, size_t n, size_t chunk_len,
                                      uint8_t* out_commitments_be /* count x 32, may be NULL */,
                                      uint8_t* out_ys_be /* count x m x l x 32, may be NULL */,
                                      uint8_t* out_proofs_be /* count x m x 32, may be NULL */, uint64_t* bad_index /* may be NULL */);
/* The disperser's call: kzg_encode_cosets_batch_bytes with eval_form = 0 (headers are defined on coefficients) and, from the same
 * resident coefficients, the blob headers.  The outputs are those of that entry plus kzg_header_items_encode_be of
 * kzg_commit_with_length_proof_batch (g2_srs, g2_trailing, trailing_first_power, srs_order, claimed_len as there, n = poly_len) on the
 * decoded blobs, byte for byte: out_length_commitments_be and out_length_proofs_be, count x 64 each.  Per group the decoded
 * coefficients that feed the encoder also feed the batched G1 MSM and the batched G2 MSM over both base sets (which may split the
 * group further by its own rule, kzg_msm_g2_batch_info); a blob's two G2 elements come down as wire points and are compressed on the
 * host.  The three header outputs are required, out_ys_be and out_proofs_be may each be NULL.  Device memory: that of
 * kzg_encode_cosets_batch_bytes and of the G2 MSM of one group (slot 0's workspace), side by side.
 * Errors, in this order, 1 - 3 on the host before anything is launched: 1. rows 1 - 2 of kzg_encode_cosets_batch_bytes (a null
 * g2_srs, g2_trailing or header output counts as a null pointer of row 1); 2. a G2 handle of another device -> KZG_ERR_INVALID_ARG,
 * then rows 3 onward of kzg_commit_with_length_proof_batch; 3. a _begin in flight on slot 0 -> KZG_ERR_INVALID_ARG; 4. a value >= r as
 * above. */
int32_t kzg_disperse_blobs_bytes(kzg_ctx* ctx, kzg_srs* srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing,
                                 uint64_t trailing_first_power, uint64_t srs_order, const uint8_t* blobs_be /* count x d x 32 */,
                                 size_t count, size_t poly_len /* d */, size_t n, size_t chunk_len, uint64_t claimed_len,
                                 uint8_t* out_commitments_be /* count x 32 */, uint8_t* out_length_commitments_be /* count x 64 */,
                                 uint8_t* out_length_proofs_be /* count x 64 */, uint8_t* out_ys_be /* count x m x l x 32, may be NULL */,
                                 uint8_t* out_proofs_be /* count x m x 32, may be NULL */, uint64_t* bad_index /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
