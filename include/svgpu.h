/*
 * svgpu.h -- C ABI of the MI355X-native BN254 MSM + KZG-decider backend (libsvgpu.so).
 *
 * Drop-in boundary for snark-verifier's native hot path (yuliakot/snark-verifier-axiom):
 *
 *   sv_bn254_g1_msm          replaces  NativeLoader::multi_scalar_multiplication
 *                                      snark-verifier/src/loader/native.rs:61-71
 *                            and       util::msm::multi_scalar_multiplication
 *                                      snark-verifier/src/util/msm.rs:287-316
 *   sv_bn254_kzg_decide      replaces  AccumulationDecider::{decide, decide_all} for KzgAs on NativeLoader
 *                                      snark-verifier/src/pcs/kzg/decider.rs:60-68 and :70-80
 *   sv_bn254_kzg_accumulate  replaces  KzgAs::create_proof's two MSMs (no zk blind)
 *   sv_bn254_kzg_create_proof   the same with r squeezed from the Poseidon transcript
 *                                      snark-verifier/src/pcs/kzg/accumulation.rs:146-195
 *                                      (also AccumulationScheme::verify, :40-62)
 *
 * The Rust binding a maintainer adds is in INTEGRATION.md.  Conventions:
 *  - every function is extern "C", never throws, and returns an sv_status;
 *  - every pointer is caller-owned and borrowed for the call only; nothing is retained;
 *  - field elements are 4 x u64 little-endian limbs (= halo2curves' in-memory Fq/Fr layout);
 *    `form` says whether inputs/outputs are canonical (SV_CANONICAL) or Montgomery with
 *    R = 2^256 (SV_MONTGOMERY, zero-copy with halo2curves memory);
 *  - the affine identity is (0, 0), as halo2curves encodes it;
 *  - calls are re-entrant: each call draws a workspace (scratch, events, a stream of its own) from
 *    a per-device pool.
 *  - Streams.  Every `*_device` entry point takes `void* stream`, a hipStream_t of `device` (of the
 *    handle's device where there is no `device` argument).  NULL means that device's legacy
 *    default stream (hipStream_t 0, the stream PyTorch calls the default stream).
 *    1. Ordered after the caller's stream: everything enqueued on `stream` before the call
 *       happens-before every read and every write the call makes through its device pointers --
 *       inputs that earlier work produces (read after write) and outputs that earlier work still
 *       reads (write after read).  With a non-NULL stream the call's work runs on that stream.
 *       With NULL it runs on the workspace's own non-blocking stream, made to wait for an event
 *       recorded on the legacy default stream when the call starts (nothing is recorded when
 *       that stream is found idle): the library never launches on the default stream itself, so
 *       concurrent callers do not serialise against each other or against the device's blocking
 *       streams.
 *    2. Synchronous: every entry point except the two named in 3 returns with its outputs
 *       complete, device outputs included ("synchronous on `stream`").  Given 1, all work
 *       enqueued on `stream` before the call has then completed as well.
 *    3. sv_bn254_poseidon_permute_device and sv_bn254_poseidon_squeeze_device are asynchronous:
 *       their kernel is enqueued on `stream` itself (NULL: on the legacy default stream) and the
 *       call returns at once.  The results are ordered for later work on the same stream; the
 *       host reads them after synchronising that stream.
 *    4. Not supported: stream capture (hipStreamBeginCapture / graphs: the calls synchronise), and
 *       a `stream` that belongs to another device than the call's.
 *    The host-buffer entry points take no stream: they read and write host memory only and are
 *    synchronous.
 *  - there is NO CPU fallback inside this library: without a usable GPU every compute entry
 *    point returns SV_ERR_DEVICE (the Rust shim then keeps the reference's own CPU code path).
 */
#ifndef SVGPU_H_
#define SVGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define SV_NOEXCEPT noexcept
extern "C" {
#else
#define SV_NOEXCEPT
#endif

#define SVGPU_ABI_VERSION 1

typedef struct { uint64_t l[4]; } sv_fe;                 /* Fq or Fr element                     */
typedef struct { sv_fe x, y; } sv_g1_affine;             /* identity = all-zero                  */
typedef struct { sv_fe x, y, z; } sv_g1_jacobian;        /* x = X/Z^2, y = Y/Z^3; identity Z = 0 */
typedef struct { sv_fe c0, c1; } sv_fq2;                 /* c0 + c1*u, u^2 = -1                  */
typedef struct { sv_fq2 x, y; } sv_g2_affine;            /* D-type twist coords; identity = 0    */
typedef struct { sv_fq2 c[6]; } sv_fq12;                 /* c0.c0 c0.c1 c0.c2 c1.c0 c1.c1 c1.c2  */

enum sv_form { SV_CANONICAL = 0, SV_MONTGOMERY = 1 };

enum sv_status {
  SV_OK = 0,
  SV_ERR_EMPTY = 1,  /* n == 0: "pairs should not be empty" (native.rs:69) / decider.rs:74 */
  SV_ERR_LEN = 2,    /* size too large for the device workspace                            */
  SV_ERR_ARG = 3,    /* null pointer, bad form, non-reduced element, point not on curve    */
  SV_ERR_DEVICE = 4, /* no usable GPU, or a HIP runtime error                              */
  SV_ERR_OOM = 5     /* device allocation failed                                           */
};

/* ---- runtime ---------------------------------------------------------------------- */
int sv_init(int num_devices) SV_NOEXCEPT;        /* idempotent; <= 0 means every visible device      */
int sv_device_count(void) SV_NOEXCEPT;           /* devices initialised (0 before sv_init / no GPU)  */
const char* sv_last_error(void) SV_NOEXCEPT;     /* thread-local message for the last non-OK status  */
const char* sv_version(void) SV_NOEXCEPT;

/* ---- a1/a3: multi-scalar multiplication ---------------------------------------------
 * out = sum_i scalars[i] * bases[i] as an affine point (identity -> (0,0)).
 * Host buffers.  num_gpus <= 0 means every initialised device (point-sharded, partials
 * folded in device order).  Scalars must be reduced (< r) and base coordinates reduced
 * (< p) in the given form, else SV_ERR_ARG.  The inputs reach HBM in pieces on a copy
 * stream (default: 4 pieces weighted 5,4,4,3 from 2^18 points, 2 equal from 2^15, else 1;
 * SVGPU_H2D_PIECES = N equal pieces, SVGPU_H2D_SPLIT = comma-separated weights); each
 * piece is sorted on a second stream once its scalars land and accumulated into the one
 * bucket set once its bases land, while later pieces are in flight; buffers are pooled.   */
int sv_bn254_g1_msm(const sv_g1_affine* bases, const sv_fe* scalars, size_t n, int form,
                    int num_gpus, sv_g1_affine* out) SV_NOEXCEPT;

/* The same MSM over the exact shape NativeLoader::multi_scalar_multiplication receives
 * (native.rs:61-71: pairs: &[(&Fr, &G1Affine)], an array of references into scattered
 * caller memory).  The library gathers the referenced 96 B per pair on its host worker pool
 * straight into pinned staging, piece by piece, and each piece's DMA and sort overlap the
 * gather of the next -- the shim passes its pairs as this 16-B-per-pair struct array (a Rust
 * tuple's field order is unspecified, so the shim maps (&Fr, &G1Affine) into sv_msm_ref).
 * A NULL reference is SV_ERR_ARG.                                                          */
typedef struct { const sv_fe* scalar; const sv_g1_affine* base; } sv_msm_ref;
int sv_bn254_g1_msm_refs(const sv_msm_ref* pairs, size_t n, int form, int num_gpus,
                         sv_g1_affine* out) SV_NOEXCEPT;

/* Device-resident variant (bases/scalars already in HBM on `device`, `stream` may be NULL):
 * writes this shard's partial sum to *out_partial (host memory, Jacobian, canonical form).
 * This is the per-rank step of the RCCL-sharded MSM (one process per GPU).              */
int sv_bn254_g1_msm_device(const sv_g1_affine* d_bases, const sv_fe* d_scalars, size_t n,
                           int form, int device, void* stream, sv_g1_jacobian* out_partial) SV_NOEXCEPT;

/* Fold Jacobian partials (canonical form) in index order and convert to affine.  Host-only
 * (no GPU needed): the combine step after the RCCL all-gather of per-rank partials.      */
int sv_bn254_g1_fold(const sv_g1_jacobian* partials, size_t k, sv_g1_affine* out, int out_form) SV_NOEXCEPT;

/* ---- a7/a8: KZG decider ----------------------------------------------------------------
 * For every i: e(lhs[i], g2) * e(rhs[i], -s_g2) == 1 ?  *first_fail = first failing index, or
 * -1 when all pass (the reference returns Err(AssertionFailure) on the first failure).
 * Identity G1 inputs contribute 1, as halo2curves' multi_miller_loop skips them.          */
int sv_bn254_kzg_decide(const sv_g2_affine* g2, const sv_g2_affine* s_g2,
                        const sv_g1_affine* lhs, const sv_g1_affine* rhs, size_t n, int form,
                        int num_gpus, int32_t* first_fail) SV_NOEXCEPT;

/* Device-resident variant; optional per-accumulator outputs:
 *   verdicts (host, n int32: 1 = pass) and gt (host, n sv_fq12, canonical: the value
 *   e(lhs,g2)*e(rhs,-s_g2) after final exponentiation, for Gt-value parity tests).        */
int sv_bn254_kzg_decide_device(const sv_g2_affine* g2, const sv_g2_affine* s_g2,
                               const sv_g1_affine* d_lhs, const sv_g1_affine* d_rhs, size_t n,
                               int form, int device, void* stream, int32_t* first_fail,
                               int32_t* verdicts, sv_fq12* gt) SV_NOEXCEPT;

/* ---- a10: KZG accumulation (KzgAs::create_proof / verify without blind) -----------------
 * out_lhs = sum_i r^i lhs[i], out_rhs = sum_i r^i rhs[i], r^0 = 1 (loader.rs:71-78).       */
int sv_bn254_kzg_accumulate(const sv_g1_affine* lhs, const sv_g1_affine* rhs, size_t n,
                            const sv_fe* r, int form, int num_gpus, sv_g1_affine* out_lhs,
                            sv_g1_affine* out_rhs) SV_NOEXCEPT;

/* KzgAs::create_proof without blind, challenge included (accumulation.rs:146-195): a fresh
 * Poseidon transcript (T = 3, RATE = 2, R_F = 8, R_P = 57, snark-verifier-sdk/src/halo2.rs:52-55)
 * absorbs lhs[i], rhs[i] for i = 0..n through common_ec_point (x, y as Fq -> Fr mod r,
 * system/halo2/transcript/halo2.rs:214-226), squeezes r (accumulation.rs:176), then returns the
 * sv_bn254_kzg_accumulate result for that r.  sponge_state (3 elements in `form`, may be
 * NULL = a fresh transcript, Poseidon::new's (2^64, 0, 0)) is the transcript's sponge state before
 * the call and receives it after the squeeze, for a transcript that was squeezed before (its
 * buffer empty).  out_r (may be NULL) receives r in `form`.  An identity accumulator point is
 * SV_ERR_ARG (the reference's Error::Transcript, halo2.rs:215-223).  The sponge (n + 1 dependent
 * permutations) runs on the host; the MSMs on the device.                                    */
int sv_bn254_kzg_create_proof(const sv_g1_affine* lhs, const sv_g1_affine* rhs, size_t n, int form,
                              int num_gpus, sv_g1_affine* out_lhs, sv_g1_affine* out_rhs,
                              sv_fe* sponge_state, sv_fe* out_r) SV_NOEXCEPT;

/* ---- batched small MSMs -------------------------------------
 * count independent MSMs over shared arrays: MSM k = sum_{i in [offsets[k], offsets[k+1])}
 * scalars[i] * bases[i]; offsets has count + 1 non-decreasing entries; out[k] affine in
 * `form`.  The per-proof Msm::evaluate calls of a native verifier (bdfg21.rs:75-78,
 * gwc19.rs:76-79 -> native.rs:61-71) and the two accumulation MSMs of KzgAs::create_proof
 * (accumulation.rs:177-192) in one launch.  An empty MSM is SV_ERR_EMPTY ("pairs should not
 * be empty", native.rs:69).  Host API: MSMs above SVGPU_BATCH_MAX terms (default 4096), and
 * every MSM of a batch of at most SVGPU_BATCH_SEQ_MAX (default 4), run through the single-MSM
 * pipeline instead.  Device API: every MSM runs in the batch kernel
 * (max_terms = the largest MSM, picks the window size); synchronous on `stream`.          */
int sv_bn254_g1_msm_batch(const sv_g1_affine* bases, const sv_fe* scalars, const uint64_t* offsets,
                          size_t count, int form, sv_g1_affine* out) SV_NOEXCEPT;
int sv_bn254_g1_msm_batch_device(const sv_g1_affine* d_bases, const sv_fe* d_scalars,
                                 const uint64_t* d_offsets, size_t count, size_t max_terms,
                                 int form, int device, void* stream,
                                 sv_g1_affine* d_out) SV_NOEXCEPT;

/* ---- device-resident fixed bases for batched MSMs ------------
 * A native verifier's constant bases -- the generator and the circuit's preprocessed
 * commitments, loaded once per verifier (Protocol::loaded, plonk/protocol.rs:106-131; used by
 * the per-proof Msm::evaluate of bdfg21.rs:75-78 / gwc19.rs:76-79) -- are uploaded ONCE as a
 * base table (stored in Montgomery form on `device`; coordinates must be reduced) and then
 * referenced by index, so a per-proof batch ships only scalars and u32 indices:
 *   MSM k = sum_{i in [offsets[k], offsets[k+1])} scalars[i] * table[base_idx[i]].
 * An index >= the table length is SV_ERR_ARG; an empty MSM is SV_ERR_EMPTY.  Handles are
 * process-wide and thread-safe; a destroyed or unknown handle is SV_ERR_ARG.              */
int sv_bn254_g1_table_create(const sv_g1_affine* bases, size_t n, int form, int device,
                             uint64_t* handle) SV_NOEXCEPT;
int sv_bn254_g1_table_destroy(uint64_t handle) SV_NOEXCEPT;
int sv_bn254_g1_msm_batch_table(uint64_t handle, const uint32_t* base_idx, const sv_fe* scalars,
                                const uint64_t* offsets, size_t count, int form,
                                sv_g1_affine* out) SV_NOEXCEPT;
/* Table rows are precomputed at creation as their window multiples 2^(8 w) P (w < 32, affine,
 * 2 KiB per row on the device), so a table-backed MSM puts every signed 8-bit digit of every
 * term into ONE bucket set (no per-MSM Horner over windows).  Device-buffer form of the same:
 * d_base_idx / d_scalars / d_offsets (count + 1 entries) / d_out on the table's device
 * (sv_bn254_g1_table_device), synchronous on `stream`; an empty MSM gives the identity.     */
int sv_bn254_g1_msm_batch_table_device(uint64_t handle, const uint32_t* d_base_idx, const sv_fe* d_scalars,
                                       const uint64_t* d_offsets, size_t count, int form, void* stream,
                                       sv_g1_affine* d_out) SV_NOEXCEPT;
int sv_bn254_g1_table_device(uint64_t handle, int* device) SV_NOEXCEPT;
/* device-buffer form over a raw (not precomputed) table: d_table (table_len rows, `table_form`), d_base_idx / d_scalars / d_offsets /
 * d_out on `device`; max_terms = the largest MSM (picks the window size); synchronous.        */
int sv_bn254_g1_msm_batch_indexed_device(const sv_g1_affine* d_table, size_t table_len, int table_form,
                                         const uint32_t* d_base_idx, const sv_fe* d_scalars,
                                         const uint64_t* d_offsets, size_t count, size_t max_terms,
                                         int form, int device, void* stream,
                                         sv_g1_affine* d_out) SV_NOEXCEPT;

/* ---- resident base sets for large MSMs ------------------------------------------------
 * The bases of a KZG MSM are almost never new (the SRS, a Lagrange basis, a committing key): a
 * base set uploads n affine points ONCE and keeps them on one device in the form the MSM
 * pipeline consumes -- the Montgomery rows (64 B) and the accumulate's 29-bit table records of P
 * and phi(P) (144 B), 208 B per point -- so that an MSM call ships only scalars (32 B per term
 * instead of 96) and converts, checks or tabulates no base:
 *   out = sum_{i<n} scalars[i] * set[offset + i];  `form` is the scalars' and the output's form.
 * create / create_device (rows already in HBM on `device`, `stream` may be NULL): `device` is the
 * index of an initialised device, as for sv_bn254_g1_table_create; coordinates must be reduced
 * (checked on the device: SV_ERR_ARG, no handle is issued and nothing stays allocated); identity
 * rows (0, 0) are legal and contribute nothing; n > 2^26 is SV_ERR_LEN.  The caller's rows are
 * not retained.  info: rows, device index and bytes held on the device (any of the three may be
 * NULL).  msm_bases takes host scalars (fed in pieces like sv_bn254_g1_msm -- default: pieces
 * weighted 1,3,4 from 2^20 terms, 1,3 from 2^18, else one; SVGPU_H2D_PIECES / SVGPU_H2D_SPLIT
 * apply -- a piece is accumulated as soon as its own sort is done: there is no base transfer to
 * wait for), msm_bases_device scalars in HBM on the set's device and returns the
 * Jacobian partial like sv_bn254_g1_msm_device.  Checked before any device work, in this order:
 * bad form or null pointer SV_ERR_ARG, n == 0 SV_ERR_EMPTY, n > 2^26 SV_ERR_LEN, unknown or
 * destroyed handle SV_ERR_ARG (a base-table handle is not a base-set handle, nor the reverse),
 * offset + n beyond the set SV_ERR_ARG.  An unreduced scalar is SV_ERR_ARG for that call; the
 * handle stays usable.  The plan (window size, GLV, ...) follows the call's n, not the set's
 * size; calls of at most 256 terms take the small-MSM route over the set's rows.  Resident calls
 * always run the 29-bit accumulate chain (SVGPU_ACC_R29 does not apply) and fill
 * sv_msm_last_stats like the other MSM calls.
 * Handles are process-wide and thread-safe: any number of threads may run MSMs on one handle at
 * once (the set is read-only).  Destroying a handle while another thread is inside a call that
 * uses it is a caller error, as it is for base tables.
 * One handle lives on ONE device; there is no multi-device handle.  A caller with several GPUs
 * makes one set per device over its shard of the bases, calls msm_bases_device per device and
 * folds the Jacobian partials with sv_bn254_g1_fold.                                          */
int sv_bn254_g1_bases_create(const sv_g1_affine* bases, size_t n, int form, int device,
                             uint64_t* handle) SV_NOEXCEPT;
int sv_bn254_g1_bases_create_device(const sv_g1_affine* d_bases, size_t n, int form, int device,
                                    void* stream, uint64_t* handle) SV_NOEXCEPT;
int sv_bn254_g1_bases_destroy(uint64_t handle) SV_NOEXCEPT;
int sv_bn254_g1_bases_info(uint64_t handle, uint64_t* n, int* device, uint64_t* device_bytes) SV_NOEXCEPT;
int sv_bn254_g1_msm_bases(uint64_t handle, size_t offset, const sv_fe* scalars, size_t n, int form,
                          sv_g1_affine* out) SV_NOEXCEPT;
int sv_bn254_g1_msm_bases_device(uint64_t handle, size_t offset, const sv_fe* d_scalars, size_t n,
                                 int form, void* stream, sv_g1_jacobian* out_partial) SV_NOEXCEPT;

/* ---- KZG opening on a resident base set ------------------------------------------------
 * The step between a commit (sv_bn254_g1_msm_bases over the coefficients) and sv_bn254_kzg_decide:
 * for p(X) = sum_{i<n} a_i X^i and a point z, the quotient q = (p - p(z)) / (X - z) and the witness
 * sum_{i<n-1} q_i set[offset + i], with the division on the device (a three-launch suffix scan over
 * Fr, csrc/kzg_open.hip) and the witness through the resident MSM pipeline, so coefficients that are
 * already in HBM never travel to the host.  With the suffix Horner values h_i = a_i + z h_{i+1}:
 * p(z) = h_0 and q_i = h_{i+1}, all mod r, so every output is determined bit for bit.  For a set
 * set[i] = s^i g and the commitment C of p over it, lhs = C - p(z) g + z witness, rhs = witness is
 * an accumulator that sv_bn254_kzg_decide accepts under (g, g2, s g2).
 * fr_poly_div_linear_device: the division alone.  d_coeffs (n elements) and d_quotient (n - 1
 *   elements, `form`; may be NULL = evaluate only; overlapping d_coeffs is SV_ERR_ARG) are in HBM
 *   on `device` (as for sv_bn254_g1_msm_device), `stream` may be NULL; z and out_eval are host
 *   pointers; synchronous on `stream`.
 * kzg_open / kzg_open_device: coefficients on the host (one transfer) or in HBM on the set's
 *   device; the quotient lives in pooled scratch in Montgomery form and feeds the set's MSM on the
 *   same stream (sv_msm_last_stats reflects that MSM).  `form` covers the coefficients, z, the
 *   evaluation and the affine witness; the Jacobian partial is canonical, as for
 *   sv_bn254_g1_msm_bases_device.  n == 1 is legal: the evaluation is a_0, the witness the identity,
 *   and no MSM runs; an all-zero quotient gives the identity too.
 * Checked before any device work, in this order: bad form or null pointer SV_ERR_ARG, n == 0
 * SV_ERR_EMPTY, n > 2^26 SV_ERR_LEN, z not below r SV_ERR_ARG ("not reduced"), unknown or destroyed
 * handle SV_ERR_ARG, offset + (n - 1) beyond the set SV_ERR_ARG.  A coefficient not below r is
 * SV_ERR_ARG ("not reduced") for that call, found on the device; the handle stays usable.  Calls
 * are re-entrant on one handle like the other resident calls.
 * Not covered: host coefficients fed in pieces, high end first, so that the copy overlaps the scan
 * and the sort; multi-device sets.  Several polynomials at one point: the batched opening below;
 * several points: one batched opening per point (svgpu.kzg.gwc19_open groups the queries), or
 * the SHPLONK opening further down, whose two MSMs do not grow with the number of points.        */
int sv_bn254_fr_poly_div_linear_device(const sv_fe* d_coeffs, size_t n, const sv_fe* z, int form,
                                       int device, void* stream, sv_fe* d_quotient,
                                       sv_fe* out_eval) SV_NOEXCEPT;
int sv_bn254_kzg_open(uint64_t handle, size_t offset, const sv_fe* coeffs, size_t n, const sv_fe* z,
                      int form, sv_fe* out_eval, sv_g1_affine* out_witness) SV_NOEXCEPT;
int sv_bn254_kzg_open_device(uint64_t handle, size_t offset, const sv_fe* d_coeffs, size_t n,
                             const sv_fe* z, int form, void* stream, sv_fe* out_eval,
                             sv_g1_jacobian* out_witness_partial) SV_NOEXCEPT;

/* ---- batched KZG opening on a resident base set: one GWC19 point set per call -----------
 * GWC19 (snark-verifier/src/pcs/kzg/multiopen/gwc19.rs:43-80) groups its queries by point and
 * takes ONE witness per point set: for the m polynomials p_j opened at z and a challenge v,
 *   c = sum_j v^j p_j (v^0 = 1),  e_j = p_j(z),  q = (c - c(z)) / (X - z),
 *   witness = sum_{k<N-1} q_k set[offset + k],  N = max lens[j]
 * (a shorter polynomial is zero past its end).  One pass over the polynomials gives c and every
 * e_j (each polynomial is read once; csrc/kzg_open.hip), the division above runs over c, and ONE
 * MSM of the set gives the witness, where m single openings run m.  All mod r and a group sum:
 * every output is determined bit for bit.
 * d_polys and lens are HOST arrays of m device pointers and lengths; each polynomial lives on
 * the set's device (or on `device`), 16-byte aligned, in `form`; a pointer may appear more than
 * once; inputs are only read.  `form` covers the coefficients, z, v, the evaluations (out_evals:
 * m host elements) and d_combined; the Jacobian partial is canonical.  `stream` may be NULL.
 * fr_poly_combine_eval_device: c and the e_j alone.  d_combined (N elements in HBM; may be NULL =
 *   evaluate only) must not overlap a polynomial ("overlaps", SV_ERR_ARG).
 * kzg_open_batch_device: the opening.  c and q live in pooled scratch in Montgomery form beside
 *   the per-call table (pointers, lengths, powers of v: one small copy on the call's stream).
 *   N == 1 runs no MSM and gives the identity, as does an all-zero quotient (v = 0 with a constant
 *   p_0, or c == 0); sv_msm_last_stats reflects the witness MSM.
 * Checked before any device work, in this order: bad form, a null pointer (d_polys, lens, z, v,
 * out_evals, the witness pointer, any d_polys[j]) or a misaligned d_polys[j] SV_ERR_ARG; m == 0 or
 * any lens[j] == 0 SV_ERR_EMPTY; m > SV_OPEN_BATCH_MAX or any lens[j] > 2^26 SV_ERR_LEN (of a
 * longer batch only the first SV_OPEN_BATCH_MAX entries are looked at); z not below r, then v
 * SV_ERR_ARG ("not reduced"); combine_eval: d_combined misaligned or overlapping a polynomial
 * SV_ERR_ARG; opening: unknown or destroyed handle, then offset + (N - 1) beyond the set
 * SV_ERR_ARG.  A coefficient not below r is SV_ERR_ARG ("not reduced") for that call, found on the
 * device; the handle stays usable and nothing is retained.  Calls are re-entrant on one handle.
 * The pass keeps m * ceil(N / 1024) block totals (32 B each) in scratch: 2 MiB at m = 64, N = 2^20.
 * Not covered: a batch fed from host coefficients (a caller with host coefficients uploads them
 * first); multi-device sets.  The SHPLONK (bdfg21) prover: the block after this one.            */
#define SV_OPEN_BATCH_MAX 4096 /* polynomials per call */
int sv_bn254_fr_poly_combine_eval_device(const sv_fe* const* d_polys, const uint64_t* lens, size_t m,
                                         const sv_fe* z, const sv_fe* v, int form, int device,
                                         void* stream, sv_fe* d_combined, sv_fe* out_evals) SV_NOEXCEPT;
int sv_bn254_kzg_open_batch_device(uint64_t handle, size_t offset, const sv_fe* const* d_polys,
                                   const uint64_t* lens, size_t m, const sv_fe* z, const sv_fe* v,
                                   int form, void* stream, sv_fe* out_evals,
                                   sv_g1_jacobian* out_witness_partial) SV_NOEXCEPT;

/* ---- several points: evaluation, division by several roots, the SHPLONK (bdfg21) opening ----
 * SHPLONK (snark-verifier/src/pcs/kzg/multiopen/bdfg21.rs, the SDK's default multi-open) groups
 * the polynomials into sets i = 1..s whose members p_ij are all opened at the same points z_ik,
 * k < K_i, and takes TWO witnesses whatever the number of points.  With challenges mu, gamma, z':
 *   e_ijk = p_ij(z_ik);  c_i = sum_j mu^j p_ij;  h_i = the quotient of c_i by Z_i = prod_k (X - z_ik),
 *   remainder dropped (0 when c_i has at most K_i coefficients);  h = sum_i gamma^i h_i (gamma^0 for
 *   the first set);  W = sum_k h_k set[offset + k];
 *   L = sum_i gamma^i Z_1(z') / Z_i(z') c_i - Z_1(z') h;  W' = sum_k q_k set[offset + k] for the
 *   quotient q of L by (X - z'), remainder dropped.
 * For set[k] = s^k g, lhs = f + z' W', rhs = W' is the accumulator of Bdfg21::verify (bdfg21.rs:47-79).
 * All mod r and group sums: every output is determined bit for bit.
 * fr_poly_eval_points_device: out_evals[j * K + k] = p_j(points[k]) for m polynomials in HBM and K
 *   points in ONE pass that reads every polynomial once (up to 4 points per launch, K trees folded
 *   per barrier; csrc/kzg_open.hip), where K single-point passes read them K times.  d_polys, lens
 *   as for the batched opening; points and out_evals are host arrays; points may repeat.
 * fr_poly_div_roots_device: d_quotient (n - K elements in HBM, `form`) = the quotient of the n
 *   coefficients at d_coeffs by prod_k (X - roots[k]), remainder dropped: K runs of the division
 *   above, Montgomery form in pooled scratch in between.  K == 1 is fr_poly_div_linear_device's
 *   quotient bit for bit.  Roots may repeat.
 * shplonk_quotient_device, shplonk_witness_device: the opening in two calls, because W enters the
 *   transcript before z' exists.  Polynomials are given in set order: set i owns
 *   d_polys[first_poly .. first_poly + num_polys) and points[first_point .. first_point + num_points),
 *   and the sets partition both arrays in order.  d_work is CALLER-OWNED HBM on the set's device of
 *   at least shplonk_work_elems elements (n_sets sets, N = the longest polynomial): the first call
 *   leaves c_1 .. c_s and h there in Montgomery form (private layout), the second reads them, so the
 *   library keeps no state between the calls.  The second call trusts the contents of d_work but
 *   never reads outside work_elems; set_lens[i] = N_i, the longest polynomial of set i.  d_work must
 *   not overlap a polynomial.  W takes max_i (N_i - K_i) rows of the set and no MSM when every h_i is
 *   zero (the identity); W' takes N - 1 rows, and N == 1 gives the identity.  `form` covers
 *   coefficients, points and challenges; the Jacobian partials are canonical.
 * Checked before any device work, in this order: bad form, a null pointer, a misaligned
 * d_polys[j], d_coeffs, d_quotient or d_work SV_ERR_ARG; m, K, n, n_sets or n_points == 0, any
 * length 0, a set without polynomials or points SV_ERR_EMPTY; K (of the call or of a set) >
 * SV_EVAL_POINTS_MAX, m or n_sets > SV_OPEN_BATCH_MAX, a length > 2^26 SV_ERR_LEN; a point or root,
 * then mu, gamma, z' not below r SV_ERR_ARG ("not reduced"); div_roots: n <= K, then d_quotient
 * overlapping d_coeffs SV_ERR_ARG; shplonk: sets that do not partition the arrays, two equal points
 * inside one set ("repeated point"), z' equal to a point, work_elems too small, d_work over a
 * polynomial, an unknown handle, a range beyond the set SV_ERR_ARG.  A coefficient not below r is
 * SV_ERR_ARG ("not reduced") for that call, found on the device; the handle stays usable.  Calls
 * are re-entrant on one handle and `stream` may be NULL.
 * Not covered: multi-device sets; openings fed from host coefficients; a fused division by
 * several roots (K suffix scans over one read).                                               */
#define SV_EVAL_POINTS_MAX 16 /* points per evaluation call, roots per division, points per set */
int sv_bn254_fr_poly_eval_points_device(const sv_fe* const* d_polys, const uint64_t* lens, size_t m,
                                        const sv_fe* points, size_t K, int form, int device,
                                        void* stream, sv_fe* out_evals) SV_NOEXCEPT;
int sv_bn254_fr_poly_div_roots_device(const sv_fe* d_coeffs, size_t n, const sv_fe* roots, size_t K,
                                      int form, int device, void* stream,
                                      sv_fe* d_quotient) SV_NOEXCEPT;
typedef struct { uint32_t first_poly, num_polys, first_point, num_points; } sv_shplonk_set;
int sv_bn254_shplonk_work_elems(size_t n_sets, size_t N, uint64_t* elems) SV_NOEXCEPT;
int sv_bn254_shplonk_quotient_device(uint64_t handle, size_t offset, const sv_fe* const* d_polys,
                                     const uint64_t* lens, size_t m, const sv_shplonk_set* sets,
                                     size_t n_sets, const sv_fe* points, size_t n_points,
                                     const sv_fe* mu, const sv_fe* gamma, int form, void* stream,
                                     sv_fe* d_work, uint64_t work_elems,
                                     sv_g1_jacobian* out_w_partial) SV_NOEXCEPT;
int sv_bn254_shplonk_witness_device(uint64_t handle, size_t offset, const sv_shplonk_set* sets,
                                    size_t n_sets, const sv_fe* points, size_t n_points,
                                    const uint64_t* set_lens, const sv_fe* gamma,
                                    const sv_fe* z_prime, int form, void* stream, const sv_fe* d_work,
                                    uint64_t work_elems,
                                    sv_g1_jacobian* out_w_prime_partial) SV_NOEXCEPT;

/* ---- Fr NTT on the device: forward, inverse and coset transforms ---------------------------
 * A halo2 prover holds its columns as evaluations over the 2^k domain and computes its quotient on
 * a coset of an extended domain; the openings above take coefficients.  This block is the change
 * of basis for data that is already in HBM.
 * fr_root_of_unity (host only, no GPU needed): omega_k = the reference's root_of_unity(k)
 *   (snark-verifier/src/util/arithmetic.rs:89-96) = halo2curves' Fr::ROOT_OF_UNITY =
 *   7^((r - 1) / 2^28) squared 28 - k times, in `form`; omega_0 = 1, omega_1 = r - 1; log_n > 28 is
 *   SV_ERR_ARG.
 * fr_ntt_device: with n = 2^log_n, omega = omega_log_n and g = *shift (a host pointer; NULL = 1),
 *   SV_NTT_FORWARD  out[j] = sum_{i<n} in[i] (g omega^j)^i
 *   SV_NTT_INVERSE  the exact inverse of the forward transform with the same g:
 *                   out[i] = g^-i n^-1 sum_{j<n} in[j] omega^(-i j)
 *   in natural order on both sides.  g = 1 forward is coefficients -> evaluations on the halo2
 *   domain; g != 1 is the coset form of the extended-domain quotient.  `count` transforms lie back to
 *   back: transform t occupies elements [t n, (t + 1) n) of d_in and of d_out (HBM on `device`).
 *   d_out == d_in is in place; otherwise the ranges must not overlap at all ("overlaps",
 *   SV_ERR_ARG), and the input is only read.  `form` covers the data and the shift.  All mod r:
 *   every output is determined bit for bit.  log_n == 0 is legal: a checked copy.
 *   A transform takes ceil(log_n / 10) launches (csrc/ntt.hip); with two or more the call holds one
 *   image of the data (count n elements) in pooled scratch.  Root tables: 1 MiB per device, built at
 *   the device's first call and kept, whatever log_n.
 * Checked before any device work, in this order: bad form, a direction that is neither value, a null
 * d_in or d_out, a pointer not 16-byte aligned SV_ERR_ARG; count == 0 SV_ERR_EMPTY; log_n >
 * SV_NTT_MAX_LOG or count 2^log_n > 2^28 SV_ERR_LEN; a shift not below r SV_ERR_ARG ("not reduced");
 * a shift equal to zero SV_ERR_ARG; the partial overlap SV_ERR_ARG.  An element not below r is
 * SV_ERR_ARG ("not reduced") for that call, found on the device in the first pass: d_out is then
 * unspecified, nothing outside it is written, and the next call is exact.  Points 1 and 2 of
 * "Streams" apply (ordered after `stream`, synchronous); re-entrant from any number of threads.
 * SVGPU_NTT_TILE_LOG = 1 .. 10 (read per call) lowers the widest pass for that call: a test switch
 * that makes the multi-pass paths run at tiny sizes.
 * Not covered: host buffers (a caller uploads first); G1 transforms (a Lagrange-basis base set);
 * multi-device transforms; bit-reversed orders on either side.                                 */
#define SV_NTT_MAX_LOG 26
enum { SV_NTT_FORWARD = 0, SV_NTT_INVERSE = 1 };
int sv_bn254_fr_root_of_unity(uint32_t log_n, int form, sv_fe* out) SV_NOEXCEPT;
int sv_bn254_fr_ntt_device(const sv_fe* d_in, sv_fe* d_out, uint32_t log_n, size_t count,
                           int direction, const sv_fe* shift, int form, int device,
                           void* stream) SV_NOEXCEPT;

/* ---- extended-domain quotient: coset LDE and division by X^n - 1 ---------------------------
 * The two fixed-function ends of a halo2 prover's quotient, for data that is already in HBM:
 * EvaluationDomain::coeff_to_extended going in, and divide_by_vanishing_poly, extended_to_coeff and
 * the h_pieces of vanishing::Argument::construct coming out.  The numerator between the two is the
 * next two blocks'.  Throughout n = 2^log_n, K = log_n + log_ext, omega_K = root_of_unity(K),
 * omega_e = omega_K^n = root_of_unity(log_ext), g = *shift (a host pointer, in `form`).  The library
 * holds no zeta, as it holds no delta: a halo2 caller passes g = Fr::ZETA = 7^((r - 1) / 3).
 * fr_coset_lde_device: `count` polynomials of exactly n coefficients each lie back to back in
 *   d_coeffs (count n elements); polynomial t is extended to 2^K evaluations,
 *     d_evals[t 2^K + j] = sum_{i<n} d_coeffs[t n + i] (g omega_K^j)^i,   j < 2^K, natural order.
 *   A NULL shift means 1.  log_ext == 0 is legal and equals the forward coset NTT.  The input is
 *   only read, and nothing beyond count n elements of it is ever read: no zero-padded copy exists at
 *   any point, an input index >= n is a zero that is never loaded.  The two ranges must not overlap
 *   at all ("overlaps", SV_ERR_ARG): there is no in place.
 *   Checked before any device work, in this order: bad form, a null d_coeffs or d_evals, a pointer
 *   not 16-byte aligned SV_ERR_ARG; count == 0 SV_ERR_EMPTY; log_ext > SV_EXT_LOG_MAX, K >
 *   SV_NTT_MAX_LOG or count 2^K > 2^28 SV_ERR_LEN; a shift not below r SV_ERR_ARG ("not reduced"); a
 *   shift equal to zero SV_ERR_ARG; the overlap SV_ERR_ARG.
 * fr_quotient_coeffs_device: d_numer holds N(g omega_K^j) for j < 2^K.  With t(X) = X^n - 1,
 *   q_j = N_j / t(g omega_K^j) and h the unique polynomial of degree < 2^K with h(g omega_K^j) = q_j,
 *     d_out[i] = h_i   for i < pieces n:
 *   `pieces` blocks of n coefficients, ready for sv_bn254_g1_msm_bases_device.  The higher
 *   coefficients are dropped as halo2's truncate drops them, whether or not they are zero, and
 *   nothing outside [0, pieces n) of d_out is written.  t takes only 2^log_ext values on the coset,
 *   t(g omega_K^j) = g^n omega_e^(j mod 2^log_ext) - 1: the host builds and inverts them (one field
 *   inversion) and the first pass reads a table of at most 256 elements.  d_out == d_numer is in
 *   place; any other overlap of the two ranges is "overlaps".
 *   Checked before any device work, in this order: bad form, a null d_numer, d_out or shift (a coset
 *   is required here), a pointer not 16-byte aligned SV_ERR_ARG; pieces == 0 SV_ERR_EMPTY; log_ext >
 *   SV_EXT_LOG_MAX or K > SV_NTT_MAX_LOG, then pieces > 2^log_ext SV_ERR_LEN; a shift not below r
 *   SV_ERR_ARG ("not reduced"); a shift equal to zero SV_ERR_ARG; g^(2^K) == 1 SV_ERR_ARG ("coset
 *   meets the domain": t vanishes somewhere on it; K squarings on the host); the overlap SV_ERR_ARG.
 * Both: an element not below r is SV_ERR_ARG ("not reduced") for that call, found on the device in
 * the first pass: the output is then unspecified, nothing outside it is written, and the next call
 * is exact.  Points 1 and 2 of "Streams" apply (ordered after `stream`, synchronous); re-entrant
 * from any number of threads.  SVGPU_NTT_TILE_LOG is honoured exactly as by the NTT.  `form` covers
 * the data and the shift.  All mod r: every output is determined bit for bit.
 * Scratch (pooled): the NTT's at K -- 256 B, the first pass's flags and, with two or more passes
 * (K > 10), one image of count 2^K elements -- plus, for the quotient, the table (2^log_ext x 32 B)
 * and as many bytes of pinned host memory for its one small copy on the call's stream.
 * Not covered: blinding of h; host buffers; multi-device columns; several quotients per call; a
 * check that the dropped high coefficients are zero.                                          */
#define SV_EXT_LOG_MAX 8
int sv_bn254_fr_coset_lde_device(const sv_fe* d_coeffs, sv_fe* d_evals, uint32_t log_n,
                                 uint32_t log_ext, size_t count, const sv_fe* shift, int form,
                                 int device, void* stream) SV_NOEXCEPT;
int sv_bn254_fr_quotient_coeffs_device(const sv_fe* d_numer, sv_fe* d_out, uint32_t log_n,
                                       uint32_t log_ext, size_t pieces, const sv_fe* shift,
                                       int form, int device, void* stream) SV_NOEXCEPT;

/* ---- permutation and lookup terms of the quotient numerator -----------------------------
 * The fixed-function part of the numerator that fr_quotient_coeffs_device divides: the permutation
 * argument's constraints (snark-verifier/src/system/halo2.rs:501-591) and each lookup's five
 * (:593-655), joined as :657-668 joins them, by a Horner fold in y (halo2's y, the reference's
 * alpha).  Notation as in the block above: n = 2^log_n, K = log_n + log_ext, N = 2^K, E =
 * 2^log_ext, omega_K = root_of_unity(K), g = *shift; row j of an extended column is its value at
 * X_j = g omega_K^j, natural order, as fr_coset_lde_device leaves it.  A rotation by r rows of the
 * original domain is rot(c, r)[j] = c[(j + r E) mod N], r of either sign.  Every column is N
 * elements in HBM on `device`; pointer arrays and scalars are host memory; `form` covers the
 * columns and every scalar.
 * Both calls continue one fold: acc starts as d_acc_in[j] (0 when d_acc_in is NULL), every
 * constraint c in the order listed does acc <- acc y + c[j], and d_out[j] = acc.  The gate
 * constraints come first in the reference: fr_expressions_device (the next block) folds them into
 * what a caller passes here as d_acc_in; a circuit
 * with more columns or lookups than a call takes calls again on the running accumulator.  d_out ==
 * d_acc_in is in place; any other overlap of d_out with an input column is "overlaps".  Only the zk
 * form of the reference (zk == true) is built.
 * fr_permutation_terms_device: d_cols[j] and d_sigmas[j], j < m, are the permutation columns v_j and
 *   sigma_j; s[j] is beta delta^j, passed ready-made (the library holds no delta, as with
 *   SV_FACTOR_IDENTITY); d_z[i], i < n_z = ceil(m / chunk), the running products.  last_rotation is
 *   the reference's rotation_last, -(blinding + 1), and must satisfy -n < last_rotation < 0.  A NULL
 *   shift means 1: the call does not divide, so the plain domain is legal.  Constraints, in order:
 *     1. l0 (1 - z_0)
 *     2. l_last (z_last^2 - z_last),                                      z_last = z_(n_z - 1)
 *     3. l0 (z_i - rot(z_(i-1), last_rotation)),                          i = 1 .. n_z - 1
 *     4. l_active (rot(z_i, 1) prod_j (v_j + beta sigma_j + gamma) - z_i prod_j (v_j + s_j X + gamma)),
 *        i = 0 .. n_z - 1, j over chunk i (the last chunk may be short)
 * fr_lookup_terms_device: per descriptor, in order, with z, a' = d_permuted_input, s' =
 *   d_permuted_table and the compressed A = d_input, S = d_table on the extended domain (for a
 *   column-only lookup the LDE of what the lookup's grand product consumed):
 *     1. l0 (1 - z)
 *     2. l_last (z^2 - z)
 *     3. l_active (rot(z, 1) (a' + beta) (s' + gamma) - z (A + beta) (S + gamma))
 *     4. l0 (a' - s')
 *     5. l_active (a' - s') (a' - rot(a', -1))
 * Checked before any device work, in this order (entries beyond a cap are not looked at):
 *   1. bad form                                                                        SV_ERR_ARG
 *   2. a null d_out, pointer array, entry of one, l column, s, beta, gamma or y        SV_ERR_ARG
 *   3. chunk == 0                                                                      SV_ERR_ARG
 *   4. a column (d_acc_in included) not 16-byte aligned                                SV_ERR_ARG
 *   5. m == 0 / n_lookups == 0                                                         SV_ERR_EMPTY
 *   6. log_ext > SV_EXT_LOG_MAX                                                        SV_ERR_LEN
 *   7. K > SV_NTT_MAX_LOG                                                              SV_ERR_LEN
 *   8. m > SV_TERMS_COLUMNS_MAX / n_lookups > SV_TERMS_LOOKUPS_MAX                     SV_ERR_LEN
 *   9. beta, gamma, y, an s[j] or the shift not below r               SV_ERR_ARG ("not reduced")
 *  10. a shift equal to zero                                                           SV_ERR_ARG
 *  11. last_rotation outside -n < r < 0                                                SV_ERR_ARG
 *  12. the overlaps                                                     SV_ERR_ARG ("overlaps")
 * (the lookup call has no chunk, s, shift or last_rotation: rules 3, 10 and 11 do not arise).  An
 * element not below r is found on the device and is SV_ERR_ARG ("not reduced") for that call: d_out
 * is then unspecified, nothing outside it is written, and the next call is exact.  Points 1 and 2
 * of "Streams" apply (ordered after `stream`, synchronous); re-entrant from any number of threads.
 * All mod r: every output is determined bit for bit.
 * Each call is one launch (csrc/quotient_terms.hip) that writes d_out once and holds nothing per
 * row outside registers.  Pooled scratch: the call's table of column pointers, s_j and powers of y
 * (under 9 KiB) and as many bytes of pinned host memory for its one small copy on the call's stream.
 * Not covered: the non-zk variant; host buffers; multi-device columns.                          */
#define SV_TERMS_COLUMNS_MAX 64   /* permutation columns per call, and so z columns */
#define SV_TERMS_LOOKUPS_MAX 16   /* lookups per call */
typedef struct { const sv_fe* d_z; const sv_fe* d_permuted_input; const sv_fe* d_permuted_table;
                 const sv_fe* d_input; const sv_fe* d_table; } sv_fr_lookup;
int sv_bn254_fr_permutation_terms_device(const sv_fe* const* d_cols, const sv_fe* const* d_sigmas,
                                         const sv_fe* s, size_t m, size_t chunk,
                                         const sv_fe* const* d_z, const sv_fe* d_l0,
                                         const sv_fe* d_l_last, const sv_fe* d_l_active,
                                         const sv_fe* beta, const sv_fe* gamma, const sv_fe* y,
                                         const sv_fe* shift, int32_t last_rotation,
                                         const sv_fe* d_acc_in, sv_fe* d_out, uint32_t log_n,
                                         uint32_t log_ext, int form, int device,
                                         void* stream) SV_NOEXCEPT;
int sv_bn254_fr_lookup_terms_device(const sv_fr_lookup* lookups, size_t n_lookups,
                                    const sv_fe* d_l0, const sv_fe* d_l_last,
                                    const sv_fe* d_l_active, const sv_fe* beta, const sv_fe* gamma,
                                    const sv_fe* y, const sv_fe* d_acc_in, sv_fe* d_out,
                                    uint32_t log_n, uint32_t log_ext, int form, int device,
                                    void* stream) SV_NOEXCEPT;

/* ---- expression programs: custom gates and theta-compression ------------------------------
 * The two steps of the quotient pipeline that are a circuit's own: its gate constraints (the
 * reference's gate_constraints, snark-verifier/src/system/halo2.rs:451-455, which come FIRST in the
 * fold of :657-668) and the theta-compression of a lookup's input and table expressions into A and
 * S (compress, :614-619).  Both evaluate trees of the reference's Expression<F>
 * (snark-verifier/src/verifier/plonk/protocol.rs:309-370) at every row of a set of columns; here a
 * tree is a flat postfix program over an operand stack, evaluated independently at every row j < N.
 * Notation as in the block above: n = 2^log_n, N = 2^(log_n + log_ext), E = 2^log_ext, rot(c, r)[j] =
 * c[(j + r E) mod N], r of either sign.  log_ext = 0 is the original domain, where theta-compression
 * runs.  d_cols[i], i < n_cols, and d_stores[k], k < n_stores, are N elements each in HBM on
 * `device`; the program, the pointer arrays, consts and y are host memory; `form` covers the
 * columns, the constants and y.
 * An op is { op, zero = 0, index, rotation }: index names the column (COLUMN), constant (CONST) or
 * store (STORE) and is 0 otherwise; rotation is r for COLUMN and 0 otherwise.  With b the top:
 *     COLUMN        -> rot(d_cols[index], rotation)[j]      CONST      -> consts[index]
 *     NEG    a      -> -a                                   ADD   a b  -> a + b
 *     SUB    a b    -> a - b                                RSUB  a b  -> b - a
 *     MUL    a b    -> a b
 *     FOLD   v      -> (nothing);  acc <- acc y + v         STORE v    -> (nothing);  d_stores[index][j] = v
 * acc starts as d_acc_in[j] (0 when d_acc_in is NULL) and, if the program has at least one FOLD,
 * d_out[j] = acc is written once at the end: the running accumulator of the two terms calls, so a
 * caller runs its gates through this call and passes d_out on as their d_acc_in.  d_out == d_acc_in
 * is in place.  A program with no FOLD reads none of y, d_acc_in, d_out: they may be NULL.  Each
 * store index is the target of at most one STORE.  The reference's variants map one to one:
 * Constant and Challenge are CONST (values in `form`), Polynomial(Query) is COLUMN, Negated NEG, Sum
 * ADD, Product MUL, Scaled is CONST then MUL, DistributePowers is the Horner chain of
 * protocol.rs:359-368 written with MUL and ADD, and a CommonPolynomial (l_0, l_last, l_active, X) is
 * a column the caller supplies (X_j is the coset LDE of the polynomial X).  SUB and RSUB let a
 * compiler evaluate the deeper operand first.
 * Checked before any device work, in this order (entries beyond a cap are not looked at):
 *   1. bad form                                                                        SV_ERR_ARG
 *   2. a null program, d_cols (n_cols > 0), consts (n_consts > 0), d_stores (n_stores > 0)
 *      or entry of either pointer array                                                SV_ERR_ARG
 *   3. a column, store, d_acc_in or d_out not 16-byte aligned                          SV_ERR_ARG
 *   4. n_ops == 0                                                                      SV_ERR_EMPTY
 *   5. log_ext > SV_EXT_LOG_MAX, K > SV_NTT_MAX_LOG, then n_ops, n_cols, n_consts or
 *      n_stores above its cap                                                          SV_ERR_LEN
 *   6. the program, op by op, the message naming the first offending op: an unknown opcode; a
 *      non-zero `zero` field; an index out of range for its table (non-zero on an op without
 *      one); a rotation outside -n < r < n; a non-zero rotation on any op but COLUMN; stack
 *      underflow; depth above SV_EXPR_STACK_MAX; a second STORE to one index; then, at the end,
 *      a non-empty stack; a program with neither FOLD nor STORE                        SV_ERR_ARG
 *   7. a FOLD in the program with y or d_out NULL                                      SV_ERR_ARG
 *   8. y or a constant that the program reads not below r             SV_ERR_ARG ("not reduced")
 *   9. a store that is written, or d_out, overlapping anything else passed to the call: a
 *      column, d_acc_in (the exact d_out == d_acc_in apart), another store: an output row is
 *      written while other threads still read rotated rows           SV_ERR_ARG ("overlaps")
 * An element not below r in a column the program reads (d_acc_in included) is found on the device
 * and is SV_ERR_ARG ("not reduced") for that call: the outputs are then unspecified, nothing outside
 * them is written, and the next call is exact.  A column the program never names is never
 * dereferenced.  Points 1 and 2 of "Streams" apply (ordered after `stream`, synchronous);
 * re-entrant from any number of threads.  All mod r: every output is determined bit for bit.
 * Each call is one launch (csrc/expressions.hip): one thread per row, the top of the operand stack
 * in registers and the rest in LDS, nothing per row in scratch.  Pooled scratch: the call's table
 * of pointers, constants, y and ops (under 45 KiB) and as many bytes of pinned host memory for its
 * one small copy on the call's stream.
 * Not covered: shared intermediates (no opcode keeps a value for a second use, squares or doubles:
 * a common subexpression is evaluated again, or stored and read back as a column by a second
 * call); host buffers; multi-device columns; the non-zk variant.                               */
enum { SV_EXPR_COLUMN = 0,  /* push d_cols[index][(j + rotation E) mod N]            */
       SV_EXPR_CONST  = 1,  /* push consts[index]  (constants and challenges alike)  */
       SV_EXPR_NEG    = 2,  /* a        -> -a                                        */
       SV_EXPR_ADD    = 3,  /* a b      -> a + b      (b is the top)                 */
       SV_EXPR_SUB    = 4,  /* a b      -> a - b                                     */
       SV_EXPR_RSUB   = 5,  /* a b      -> b - a                                     */
       SV_EXPR_MUL    = 6,  /* a b      -> a b                                       */
       SV_EXPR_FOLD   = 7,  /* v        -> (nothing);  acc <- acc y + v              */
       SV_EXPR_STORE  = 8 };/* v        -> (nothing);  d_stores[index][j] = v        */
typedef struct { uint8_t op; uint8_t zero; uint16_t index; int32_t rotation; } sv_fr_expr_op; /* 8 B */
#define SV_EXPR_OPS_MAX     4096
#define SV_EXPR_COLUMNS_MAX 256
#define SV_EXPR_CONSTS_MAX  256
#define SV_EXPR_STORES_MAX  16
#define SV_EXPR_STACK_MAX   8
int sv_bn254_fr_expressions_device(const sv_fr_expr_op* program, size_t n_ops,
                                   const sv_fe* const* d_cols, size_t n_cols,
                                   const sv_fe* consts, size_t n_consts,
                                   sv_fe* const* d_stores, size_t n_stores,
                                   const sv_fe* y, const sv_fe* d_acc_in, sv_fe* d_out,
                                   uint32_t log_n, uint32_t log_ext, int form,
                                   int device, void* stream) SV_NOEXCEPT;

/* ---- running products and batch inversion over Fr columns in HBM -----------------------
 * The running-product columns of a halo2 prover: the permutation argument's z (one per chunk of
 * columns) and each lookup's z, which satisfy the relations the verifier checks in
 * snark-verifier/src/system/halo2.rs:501-591 (permutation) and :593-660 (lookup),
 *   z(wX) prod_j (v_j + beta sigma_j + gamma)  =  z(X) prod_j (v_j + beta delta^j X + gamma)
 *   z(wX) (a' + beta)(s' + gamma)              =  z(X) (a + beta)(s + gamma),
 * for columns that are already on the device (csrc/grand_product.hip: two product scans and ONE
 * field inversion per call, three launches).
 * fr_grand_product_device: with num(u) = prod_{j < n_num} num[j](u) and den(u) likewise, where a
 *   factor's value at row u is x[u] + c (PLAIN), x[u] + s y[u] + c (COLUMN) or x[u] + s omega^u + c
 *   (IDENTITY),
 *     d_z[0] = z0,   d_z[i] = z0 prod_{u < i} num(u) / den(u)   for i < n,
 *   and *out_total (a host pointer, may be NULL) the same with u < n: the value a prover checks
 *   against 1, or seeds the next chunk's z0 with.  The descriptor arrays are host memory; d_x and
 *   d_y point at n elements in HBM on `device`.  `form` covers the columns, s, c, z0, omega, d_z and
 *   out_total.  omega is read only when a factor is IDENTITY and is then required: the caller passes
 *   the domain's root_of_unity(k); s lets the caller pass beta delta^j ready-made, so the library
 *   holds no delta.  The s of a PLAIN factor and the d_y of any factor but COLUMN are not read.  n
 *   need not be a power of two.  n_den == 0 is a plain prefix product and runs no inversion; n_num
 *   == 0 is legal too.  A row whose denominator is zero contributes the ratio 0 / 1: every later z
 *   and the total are 0, which is what halo2's batch inversion gives (it leaves a zero "inverse"
 *   zero).  All mod r: every output is determined bit for bit.
 * fr_batch_invert_device: d_out[i] = 1 / d_in[i], and 0 where d_in[i] == 0 (halo2's batch
 *   inversion, and ScalarLoader::batch_invert's unwrap_or_else, snark-verifier/src/loader.rs:241-247).
 *   d_out == d_in is in place; any other overlap is SV_ERR_ARG ("overlaps").
 * Checked before any device work, in this order (a side's descriptors beyond the first
 * SV_PRODUCT_FACTORS_MAX are not looked at):
 *   1. bad form; a null d_z, z0, descriptor array with a non-zero count, d_x, or d_y of a COLUMN
 *      factor; a kind that is none of the three; a column or d_z not 16-byte aligned   SV_ERR_ARG
 *   2. n == 0, or n_num + n_den == 0                                                   SV_ERR_EMPTY
 *   3. n > 2^26, or a count above SV_PRODUCT_FACTORS_MAX                               SV_ERR_LEN
 *   4. z0, an s or c that is read, or omega (when read) not below r   SV_ERR_ARG ("not reduced")
 *   5. an IDENTITY factor with omega == NULL                                           SV_ERR_ARG
 *   6. d_z overlapping any column                                       SV_ERR_ARG ("overlaps")
 * (batch inversion: bad form, null, alignment; n == 0; n > 2^26; the partial overlap).  An element
 * not below r is found on the device and is SV_ERR_ARG ("not reduced") for that call: d_z (d_out) is
 * then unspecified, nothing outside it is written, and the next call is exact.  Points 1 and 2 of
 * "Streams" apply (ordered after `stream`, synchronous); re-entrant from any number of threads.
 * A grand product holds its rows' two products in pooled scratch between its first and its last
 * launch: 64 B per row (4 GiB at n = 2^26), so the columns are read once; batch inversion holds
 * nothing per row.
 * Not covered: several z columns in one call; host buffers; multi-device columns (a lookup's
 * permuted columns: the next block).                                                          */
enum { SV_FACTOR_PLAIN = 0,      /* f[i] = x[i] + c              */
       SV_FACTOR_COLUMN = 1,     /* f[i] = x[i] + s*y[i] + c     */
       SV_FACTOR_IDENTITY = 2 }; /* f[i] = x[i] + s*omega^i + c  */
typedef struct { const sv_fe* d_x; const sv_fe* d_y; sv_fe s; sv_fe c; uint32_t kind; } sv_fr_factor;
#define SV_PRODUCT_FACTORS_MAX 16   /* per side */
int sv_bn254_fr_grand_product_device(const sv_fr_factor* num, size_t n_num,
                                     const sv_fr_factor* den, size_t n_den, size_t n,
                                     const sv_fe* z0, const sv_fe* omega, int form, sv_fe* d_z,
                                     sv_fe* out_total, int device, void* stream) SV_NOEXCEPT;
int sv_bn254_fr_batch_invert_device(const sv_fe* d_in, sv_fe* d_out, size_t n, int form,
                                    int device, void* stream) SV_NOEXCEPT;

/* ---- Fr sort and the permuted columns of a lookup in HBM ---------------------------------
 * The a' and s' that the lookup relation above reads, from the compressed input expression A and
 * table expression S of a lookup, for columns that are already on the device
 * (csrc/lookup_permute.hip: a least-significant-digit radix sort over the canonical 256-bit value
 * in 8-bit digits, dead digits skipped, and a lower bound plus two scans).  Order is by canonical
 * integer value in [0, r) -- what Ord on halo2curves' Fr compares -- whatever `form` the data is in.
 * fr_sort_device: d_out = d_in sorted ascending (stable, though equal elements cannot be told
 *   apart), in `form`.  d_out == d_in is in place; any other overlap is SV_ERR_ARG ("overlaps").
 *   n need not be a power of two.
 * fr_lookup_permute_device: halo2's permute_expression_pair (halo2_proofs
 *   src/plonk/lookup/prover.rs) over n usable rows; the blinding rows after them are the caller's
 *   and are never touched.
 *     1. A' = A sorted ascending.  Row i of A' is a leader if i == 0 or A'[i] != A'[i-1], otherwise a
 *        repeat.
 *     2. Every leader's value must occur in S; S'[i] = A'[i] at every leader.
 *     3. L[0..m) = S with one copy of each distinct value of A removed, ascending with multiplicity
 *        (m = the number of repeats); the repeats r_0 < .. < r_{m-1} take S'[r_k] = L[m-1-k]: the
 *        smallest leftover goes to the LAST repeated row, as halo2's pop() does.
 *   The output satisfies a'[0] = s'[0], a'[i] = s'[i] or a'[i] = a'[i-1] on every row, and
 *   prod (a + beta)(s + gamma) = prod (a' + beta)(s' + gamma), bit for bit as halo2 arranges it.
 *   The inputs are only read.  Any overlap between an output and an input, or between the two
 *   outputs, is SV_ERR_ARG ("overlaps").  A leader whose value is not in S: SV_ERR_ARG ("not in
 *   table") and *out_missing_row = the SMALLEST such row of A' (where halo2 returns
 *   ConstraintSystemFailure); out_missing_row is a host pointer, may be NULL, and is UINT64_MAX on
 *   success.  The outputs are unspecified after a failure.
 * Checked before any device work, in this order:
 *   1. bad form; a null column; a pointer not 16-byte aligned                          SV_ERR_ARG
 *   2. n == 0                                                                          SV_ERR_EMPTY
 *   3. n > 2^26                                                                        SV_ERR_LEN
 *   4. the overlaps above                                               SV_ERR_ARG ("overlaps")
 * An element not below r is found on the device and is SV_ERR_ARG ("not reduced") for that call
 * (it wins over a missing value): the outputs are then unspecified, nothing outside them is
 * written, and the next call is exact.  Points 1 and 2 of "Streams" apply (ordered after `stream`,
 * synchronous); re-entrant from any number of threads.  Pooled scratch per row: 65 B for a sort
 * (two canonical images and the per-block digit counts), 145 B for a permutation (four images, four
 * u32 lists, the counts): 9.1 GiB at n = 2^26.
 * Not covered: the blinding rows; host buffers; multi-device columns.                          */
int sv_bn254_fr_sort_device(const sv_fe* d_in, sv_fe* d_out, size_t n, int form, int device,
                            void* stream) SV_NOEXCEPT;
int sv_bn254_fr_lookup_permute_device(const sv_fe* d_input, const sv_fe* d_table, size_t n,
                                      int form, sv_fe* d_permuted_input, sv_fe* d_permuted_table,
                                      uint64_t* out_missing_row, int device,
                                      void* stream) SV_NOEXCEPT;

/* ---- Batched lookup permutation: the lookups of a circuit in one call ---------------------
 * fr_lookup_permute_batch_device: `count` lookups over n usable rows each.  The four pointer
 *   arrays are HOST arrays of `count` device pointers, each to n elements on `device`.  For every
 *   lookup j, d_permuted_inputs[j] and d_permuted_tables[j] take exactly the bytes that
 *   fr_lookup_permute_device(d_inputs[j], d_tables[j], n, form, ..) writes (steps 1-3 above); the
 *   lookups are independent of each other.  The number of kernel launches does not depend on count:
 *   every column of the call is a grid row of one set of launches (104 kernels and two memsets; 105
 *   with SV_LOOKUP_TABLES_SORTED), where `count` single calls are 202 each.
 *   Tables: entries of d_tables may be equal pointers, and a table that several lookups name is
 *   read, converted and sorted ONCE per call.  Tables are deduplicated by pointer value only:
 *   distinct pointers are distinct tables, and two of them may overlap (tables are only read).
 *   Inputs are only read too; one input pointer may appear in several lookups.
 *   flags = SV_LOOKUP_TABLES_SORTED: every table of the call is already in ascending canonical
 *   order in `form` -- what fr_sort_device writes; a fixed table is the same for every proof, so
 *   it can be sorted once per circuit.  The call then sorts no table: one pass converts it and
 *   checks T[i-1] <= T[i] on the device, equal neighbours being legal; a violation is SV_ERR_ARG
 *   ("table not sorted").
 *   Failure: a leader of lookup j whose value is not in its table is SV_ERR_ARG ("not in table");
 *   out_missing_rows[j] (a host array of count entries, may be NULL) is the smallest such row of
 *   A'_j, or UINT64_MAX for a lookup that is fine, and *out_failed (host, may be NULL) the smallest
 *   failing j, or UINT64_MAX.  The outputs of the lookups that did not fail are still exact.
 * Checked before any device work, in this order:
 *   1. bad form; an unknown flag bit; a null array; a null entry; an entry not 16-byte aligned
 *                                                                                      SV_ERR_ARG
 *   2. count == 0 or n == 0                                                            SV_ERR_EMPTY
 *   3. count > SV_LOOKUP_BATCH_MAX or n > 2^26                                         SV_ERR_LEN
 *   4. an output overlapping an input, a table or another output            SV_ERR_ARG ("overlaps")
 * Rule 1 looks at all `count` entries of the four arrays before rule 3 looks at `count`: the arrays
 * must really hold `count` entries, also in a call that is then refused with SV_ERR_LEN.
 * An element not below r, in any input or table, is found on the device and is SV_ERR_ARG ("not
 * reduced"); it wins over the other two device errors, ALL outputs are then unspecified, nothing
 * outside them is written, and the next call is exact.  "table not sorted" wins over "not in
 * table"; out_missing_rows and out_failed are written only by a call that returns SV_OK or "not in
 * table".  Points 1 and 2 of "Streams" apply (ordered after `stream`, synchronous, one read-back of
 * the lookups' heads at the end); re-entrant from any number of threads.  Pooled scratch per row:
 * 65 B per sorted column (every input, and every distinct table unless the flag is set: two
 * canonical images and the per-block digit counts), 16 B per lookup (four u32 lists), 32 B per
 * table with the flag set (one image); a failed allocation is SV_ERR_OOM with nothing launched.
 * Not covered: several z columns per grand-product call; the blinding rows; host buffers;
 * multi-device columns; a public batched sort.                                                 */
#define SV_LOOKUP_BATCH_MAX 16 /* lookups per call (= SV_TERMS_LOOKUPS_MAX) */
enum { SV_LOOKUP_TABLES_SORTED = 1 }; /* flags */
int sv_bn254_fr_lookup_permute_batch_device(const sv_fe* const* d_inputs, const sv_fe* const* d_tables,
                                            size_t count, size_t n, int form, uint32_t flags,
                                            sv_fe* const* d_permuted_inputs,
                                            sv_fe* const* d_permuted_tables,
                                            uint64_t* out_missing_rows, uint64_t* out_failed,
                                            int device, void* stream) SV_NOEXCEPT;

/* ---- Poseidon sponge over BN254 Fr --------------------------
 * x^5 HADES permutation, width t = 3 (R_F 8, R_P 57, rate 2: the SDK's PoseidonTranscript,
 * snark-verifier-sdk/src/halo2.rs:52-71) or t = 5 (R_F 8, R_P 60, rate 4).  States are t
 * consecutive sv_fe; inputs must be reduced field elements.
 * permute: the bare HADES permutation of n states, in place: Poseidon::permutation
 *          (snark-verifier/src/util/hash/poseidon.rs:469-500) called with a full-rate zero
 *          input, exactly as the reference KATs call it (poseidon/tests.rs:34-85).
 * squeeze: Poseidon::squeeze (poseidon.rs:455-467) on n independent sponges.  states (n x t,
 *          in/out) are the sponges' states -- Poseidon::new starts one at (2^64, 0, ..),
 *          poseidon.rs:335-342 -- and sponge j's buffer (what Poseidon::update collected,
 *          poseidon.rs:449-452) is elements[offsets[j] .. offsets[j+1]); offsets has n + 1
 *          non-decreasing entries.  out[j] (optional, may be NULL) = the challenge state[1].  */
int sv_bn254_poseidon_permute(sv_fe* states, size_t n, int t, int form) SV_NOEXCEPT;
int sv_bn254_poseidon_permute_device(sv_fe* d_states, size_t n, int t, int form, int device,
                                     void* stream) SV_NOEXCEPT;
int sv_bn254_poseidon_squeeze(sv_fe* states, const sv_fe* elements, const uint64_t* offsets,
                              size_t n, int t, int form, sv_fe* out) SV_NOEXCEPT;
int sv_bn254_poseidon_squeeze_device(sv_fe* d_states, const sv_fe* d_elements,
                                     const uint64_t* d_offsets, size_t n, int t, int form,
                                     sv_fe* d_out, int device, void* stream) SV_NOEXCEPT;

/* ---- codecs around the path, decoded on the device --------
 * Point encodings:
 *   SV_ENC_HALO2_COMPRESSED  32 B: x little-endian, parity of y in bit 255, identity = zeros
 *                            (halo2curves GroupEncoding, read by PoseidonTranscript::read_ec_point,
 *                            system/halo2/transcript/halo2.rs:247-260)
 *   SV_ENC_EVM               64 B: x || y big-endian, identity = zeros
 *                            (EvmTranscript::read_ec_point, system/halo2/transcript/evm.rs:223-242)
 * g1_decode: n encoded points -> affine in `form`.  All valid: SV_OK and *first_invalid = -1.
 *   Otherwise SV_ERR_ARG ("Invalid elliptic curve point encoding in proof"), *first_invalid =
 *   the lowest invalid index, and invalid points are written as (0, 0).
 * accumulators_from_limbs: LimbsEncoding<LIMBS, BITS>::from_repr (pcs/kzg/accumulator.rs:57-77)
 *   for n accumulators of 4 * n_limbs Fr limbs each (lhs.x, lhs.y, rhs.x, rhs.y; fe_from_limbs,
 *   util/arithmetic.rs:262-274; the SDK uses LIMBS = 3, BITS = 88).  `form` applies to the limbs
 *   and the output.  A coordinate >= p or >= 2^256, or a point off the curve (the reference's
 *   unwrap panics) gives SV_ERR_ARG with *first_invalid = that accumulator.
 * kzg_decide_eip197: n_checks 0x180-byte ecPairing (EIP-197) inputs as the EVM decider lays them
 *   out (pcs/kzg/decider.rs:107-127, loader/evm/loader.rs:338-382): lhs, g2, rhs, -s_g2 with G2
 *   words (x.c1, x.c0, y.c1, y.c0).  All records must carry the same G2 pair (one deciding key).
 *   *first_fail = first check whose pairing product is not 1 or whose G1 encoding is invalid
 *   (the precompile would fail either way), -1 if all pass.                             */
enum { SV_ENC_HALO2_COMPRESSED = 0, SV_ENC_EVM = 1 };
int sv_bn254_g1_decode(const uint8_t* data, size_t n, int encoding, int form, sv_g1_affine* out,
                       int64_t* first_invalid) SV_NOEXCEPT;
int sv_bn254_g1_decode_device(const uint8_t* d_data, size_t n, int encoding, int form, int device,
                              void* stream, sv_g1_affine* d_out,
                              int64_t* first_invalid) SV_NOEXCEPT;
int sv_bn254_kzg_accumulators_from_limbs(const sv_fe* limbs, size_t n, int n_limbs, int bits,
                                         int form, sv_g1_affine* lhs, sv_g1_affine* rhs,
                                         int64_t* first_invalid) SV_NOEXCEPT;
int sv_bn254_kzg_decide_eip197(const uint8_t* input, size_t n_checks, int num_gpus,
                               int32_t* first_fail) SV_NOEXCEPT;

/* ---- synthetic inputs (SURVEY.md section 8d generator, index-addressable) -------------
 * Fills device buffers with the deterministic SplitMix64 scalars / try-and-increment bases
 * (elements start .. start+n-1) in the requested form.                                   */
int sv_gen_scalars_device(sv_fe* d_scalars, size_t n, uint64_t seed, uint64_t start, int form,
                          int device, void* stream) SV_NOEXCEPT;
int sv_gen_bases_device(sv_g1_affine* d_bases, size_t n, uint64_t seed, uint64_t start, int form,
                        int device, void* stream) SV_NOEXCEPT;

/* ---- instrumentation ----------------------------------------------------------------
 * Per-kernel timings (HIP events on the call's stream) of the last MSM on this thread; the digits
 * and fixup splits are filled only with SVGPU_MSM_STATS=1 (folded into sort / reduce otherwise). */
typedef struct {
  float total_ms, digits_ms, sort_ms, accumulate_ms, fixup_ms, reduce_ms, host_ms;
  uint32_t window_bits, num_windows, accumulate_launch_units;
  uint64_t entries;
  float accumulate_span_ms;        /* first accumulate launch's start to the last one's end */
  uint32_t accumulate_launches;    /* 2 when the window halves run as separate launches */
} sv_msm_stats;
int sv_msm_last_stats(sv_msm_stats* out) SV_NOEXCEPT;
/* Kernel time (HIP events on the call's stream) of the calling thread's last decider launch. */
int sv_kzg_last_kernel_ms(float* out) SV_NOEXCEPT;

#ifdef __cplusplus
}
#endif
#endif /* SVGPU_H_ */
