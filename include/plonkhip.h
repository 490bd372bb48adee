/*
 * libplonkhip -- the C ABI between the reference's host code and the gfx950 kernels.
 *
 * The reference (kazuakiishiguro/plonk.c) has no plugin/FFI layer: plonk.h calls
 * srs_eval_at_s() and poly_mul() by name after #include "srs.h" / "poly.h"
 * (src/plonk.h:8-9).  The drop-in headers in this directory keep those exact signatures and
 * route the two hot functions through the entry points below; any other host language
 * binds the same symbols (see INTEGRATION.md for the ctypes / cgo stubs).
 *
 * Conventions
 *   - plain pointers and sizes only; a G1 is 3 bytes {x, y, infinite} exactly as the
 *     reference struct (src/g1.h:8-11), an HF is 1 byte (src/hf.h:15-17);
 *   - host-buffer entry points are synchronous: results are complete on return and no
 *     caller pointer is retained;
 *   - *_dev entry points take DEVICE pointers and a hipStream_t (as void*; NULL = the HIP
 *     null stream) and are asynchronous;
 *   - every entry point returns PLK_OK (0) or a PLK_ERR_* code; plk_last_error() gives text.
 *     The drop-in headers turn a non-zero code into the reference's convention
 *     (fprintf(stderr, ...) + exit(EXIT_FAILURE), e.g. src/srs.h:54-57);
 *   - there is no CPU fallback: without a usable GPU every compute entry point fails
 *     with PLK_ERR_NODEV.  (The drop-in HEADERS keep calls of toy size on the host by their own
 *     restated code, include/plk_host.h -- SURVEY 8(b)'s small-size policy, sized by
 *     PLK_OPT_DROPIN_HOST_WORK; the library itself never computes on the CPU.)
 */
#ifndef PLONKHIP_H
#define PLONKHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PLK_OK = 0,
  PLK_ERR_HIP = 1,    /* a HIP runtime call failed */
  PLK_ERR_ARG = 2,    /* bad argument (NULL pointer, empty polynomial, ...) */
  PLK_ERR_RANGE = 3,  /* size outside what the exact algorithm supports */
  PLK_ERR_NODEV = 4,  /* no usable GPU */
  PLK_ERR_NOMEM = 5   /* device allocation failed */
};

/* ---- lifetime ------------------------------------------------------------------------ */
int plk_init(int device);            /* select device (<0: $PLK_DEVICE or 0); idempotent */
/* Several GPUs in one process (SURVEY 8(b) plk_init(n_gpus), 8(e)): ids[0] is the primary
 * device (everything runs there as after plk_init(ids[0])); plk_msm_g1 -- srs_eval_at_s, the
 * reference's commitment -- splits an MSM of at least PLK_OPT_MSM_SHARD_MIN points into n
 * contiguous point ranges, one per entry, each uploaded over its own device's link from its own
 * host thread and reduced to a partial discrete log there; the N 4-byte partials are summed
 * on the host (the result returns to the host anyway).  Ids may repeat (several shards on one
 * GPU).  Calling again replaces the list; n = 1 goes back to one device.  PLK_DEVICE="0,1,2,3"
 * does the same at implicit initialisation.  1 <= n <= 16. */
int plk_init_devices(const int *ids, int n);
int plk_devices(int *ids, int cap);  /* the shard list (or the one device); returns its length */
void plk_shutdown(void);
const char *plk_last_error(void);
int plk_device_count(void);
const char *plk_version(void);

/* ---- options --------------------------------------------------------------------------
 * Every default is the production setting; the others exist for A/B measurement and for tests
 * that force a rarely taken path.  None changes a result: every setting gives the same bytes.
 * The library reads no environment variable except PLK_DEVICE (device selection).  Options
 * marked [init] shape tables built by plk_init and may only be set before it (PLK_ERR_ARG
 * after). */
enum {
  PLK_OPT_TINY_CALLS = 1,        /* 1: toy-size host calls through mapped pinned memory; 0: staged copies */
  PLK_OPT_PROVE_SYNC = 2,        /* 0: a proof's end is seen by polling its completion word; 1: stream sync */
  PLK_OPT_POLY_BLOCK_L = 3,      /* blocked poly_mul piece lengths; 0 = the exact-range maxima       */
  PLK_OPT_POLY_BLOCK_S = 4,      /*   (both set: forces the blocked path with those pieces, >= 33)   */
  PLK_OPT_NTT_F29 = 5,           /* 1: poly_mul over F29 where exact; 0: BabyBear only                */
  PLK_OPT_NTT_SHARE = 6,         /* 1: an operand given twice in one batch is transformed once        */
  PLK_OPT_NTT_SHARED_FIX = 7,    /* 1: shared operands' lo = 0 pass in its own launch (auto), 0 off, 2 forced */
  PLK_OPT_NTT_T13_MIN_K = 8,     /* [init] 21: 2^13-element tiles from 2^k points up (13..27)        */
  PLK_OPT_NTT_CENTER_BLOCKS = 9, /* 0: resident blocks of the center kernel from the CU count        */
  PLK_OPT_MSM_THREADS = 10,      /* MSM launch geometry overrides (0 = the built-in choice):          */
  PLK_OPT_MSM_MAX_BLOCKS = 11,   /*   threads 256/512/1024, resident blocks, groups in flight 1/2/4, */
  PLK_OPT_MSM_GROUPS = 12,       /*   table copies 1/8, half groups for single MSMs (1 = on)          */
  PLK_OPT_MSM_COPIES = 13,
  PLK_OPT_MSM_HALF = 14,
  PLK_OPT_MSM_SHARD_MIN = 15,    /* multi-device plk_msm_g1: split from this many points (2^16)      */
  PLK_OPT_NTT_CENTER_SUM = 16,   /* 1: a sum group's products added in its leader's center item      */
  PLK_OPT_MSM_HOST_LANES = 17,   /* one device: plk_msm_g1 of >= MSM_SHARD_MIN points runs its SRS memcmp,
                                    staging and uploads on this many host threads (1: one); read by
                                    plk_init / plk_init_devices */
  PLK_OPT_PROVE_DERIVE_T2A = 18, /* 1: round 3's A2 B2 from a_x b_x by an elementwise pass (0: its own product;
                                    2, the default: that pass inside the t_2 product's first forward pass when
                                    it runs on 2^13 tiles -- one launch fewer -- else as 1) */
  PLK_OPT_NTT_TABLE_SHARE = 19,  /* 1: a table pass runs several arrays of one tile per block (column words read once) */
  PLK_OPT_NTT_LAUNCH_LOG = 20,   /* diagnostics: 1 records the NTT passes' launch plans (plk_ntt_launch_log) */
  PLK_OPT_PROVE_SRS_LOGS = 22,   /* 1: the prover's commitments read its SRS in log form (1 B per point,
                                    converted once at plk_prover_create); 0: the G1 form (3 B) */
  PLK_OPT_PROVE_PACK_FUSE = 23,  /* 1 (with PROVE_SRS_LOGS): commitments, trimmed lengths and the proof packing
                                    in one launch (commit_pack_kernel); 0: the MSM, then trim_pack_kernel */
  PLK_OPT_PROVE_EARLY_COMMITS = 24, /* 1 (with PROVE_PACK_FUSE): the 7 commitments that do not wait for round 5
                                       run as extra rows of round 5's fused division launch; 0: with the
                                       other two in commit_pack_kernel */
  PLK_OPT_PROVE_HELPER_COPY = 25, /* 1: helpers of plk_prover_attach_helpers on the proving device itself take
                                     the distinct-device input path (their inputs copied into their own rows,
                                     the rest pointed at a poison row): a one-GPU test of that branch */
  PLK_OPT_DROPIN_HOST_WORK = 28, /* drop-in headers (include/plk_host.h): a call whose host cost estimate (about
                                    ns: la*lb MACs for poly_mul, 300 per MSM point, ...) is at most this stays
                                    on the host; 32768 ~ one GPU round trip; 0: every call on the GPU.  The
                                    library reads it only through plk_get_option */
  PLK_OPT_DIVIDE_FAST_MIN = 29,  /* poly_divide by a general canonical divisor (not constant, not lead x^m + d0;
                                    lead in 1..16, nl >= dl): from (nl - dl + 1) * dl >= this value the
                                    quotient comes from a Newton inverse over the exact poly_mul products
                                    instead of the reference's loop on one GPU thread.  0: never, 1: whenever
                                    eligible; default 256, the measured crossover */
  /* 21, 26, 27: retired (no enumerator; set: PLK_ERR_ARG, get: -1): PROVE_FUSE_DIV, PROVE_EVAL_AGG,
     PROVE_GRAPH */
  PLK_OPT_COUNT = 30
};
int plk_set_option(int opt, int64_t value);   /* PLK_ERR_ARG: unknown option or value out of range */
/* Diagnostics for the roofline tools: with PLK_OPT_NTT_LAUNCH_LOG = 1 every NTT pass launch
 * is recorded as 8 ints {kind (0 forward, 1 inverse, 2 center, 3 shared lo = 0 pass), tile bits,
 * pass bits, log2 size, arrays / products, arrays per block, center pass units, field (0 F29,
 * 1 BabyBear)}; this copies up to cap records into out (8 ints each), clears the log and returns
 * the count. */
int plk_ntt_launch_log(int32_t *out, int cap);
int64_t plk_get_option(int opt);              /* -1 for an unknown option */

/* ---- host-buffer entry points (what the drop-in headers call) ------------------------ */

/* Replaces the body of srs_eval_at_s (src/srs.h:53-68):
 *   out = sum_{i<n} g1_mul(points[i], scalars[i]) folded left with g1_add.
 * points: n x 3 bytes, scalars: n bytes (HF.value, any byte value), out: 3 bytes.
 * The caller keeps the reference's degree check (vs->len > srs->len) before calling. */
int plk_msm_g1(const uint8_t *points, const uint8_t *scalars, size_t n, uint8_t out[3]);

/* Replaces the body of poly_mul (src/poly.h:106-122):
 *   out[0 .. la+lb-1) = a * b over GF(17); *out_len = length after the reference's
 *   trailing-zero trim (src/poly.h:20-38), >= 1.  out must hold la+lb-1 bytes.
 *   la == 0 or lb == 0 mirrors the reference: *out_len = (la+lb-1 > 0), out[0] = 0.
 *   Any shape with la + lb - 1 < 2^32: products beyond one transform's exact range
 *   (min(la, lb) >= 7,864,320 or more than 2^27 output coefficients) run as in-range piece
 *   products accumulated mod 17 (the _dev form then needs plk_poly_mul_workspace bytes). */
int plk_poly_mul(const uint8_t *a, size_t la, const uint8_t *b, size_t lb, uint8_t *out,
                 size_t *out_len);

/* ---- device-resident entry points (bench, multi-GPU, pipelines) ---------------------- */

/* Result record of one MSM, 2176 bytes of device memory.  Zero it once
 * (plk_msm_result_init); every launch leaves its internal words at zero again, so a record
 * can be reused by the next launch on the same stream.  The arrival words of the blocks of
 * one launch live on separate 128-byte lines (serialised device-scope atomics on one line
 * cost ~10 ns each: ~3 us for 256 blocks on a single word). */
typedef struct {
  uint64_t top;        /* internal: arrival word over the shards */
  uint32_t log;        /* discrete log of the result w.r.t. plk_dlog_generator(), 0..101 */
  uint32_t irregular;  /* > 0: some input was not a canonical group element -> g1 invalid,
                          run plk_msm_g1_serial_dev for the reference's exact raw fold */
  uint8_t g1[4];       /* {x, y, infinite, 0} */
  uint32_t pad[27];
  uint64_t shard[16][16]; /* internal: arrival words shard[s][0] (two per XCD): [31:0] sum,
                             [47:32] ticket, [63:48] bad; one 128-byte line each */
} plk_msm_result_t;

int plk_msm_result_init(plk_msm_result_t *d_res, void *stream);
int plk_msm_g1_dev(const uint8_t *d_points, const uint8_t *d_scalars, size_t n,
                   plk_msm_result_t *d_res, void *stream);
/* A batch of independent MSMs of n points each in ONE launch: MSM b reads
 * d_points + b * points_stride and d_scalars + b * scalars_stride and writes d_res[b].
 * (E.g. the commitments of one prover round, or many proofs' commitments at once.) */
int plk_msm_g1_batch_dev(const uint8_t *d_points, size_t points_stride, const uint8_t *d_scalars,
                         size_t scalars_stride, size_t n, int batch, plk_msm_result_t *d_res,
                         void *stream);
/* The launch plan plk_msm_g1_dev (batch = 1) / plk_msm_g1_batch_dev take for batch MSMs of n
 * points under the current options; aligned = 0: some base or stride is not 16-byte aligned.
 * out = {threads per block, blocks per MSM, groups in flight, table copies, half groups}.
 * PLK_ERR_ARG for batch <= 0 or a NULL out, PLK_ERR_RANGE for batch > 65535 (as the launch).
 * Host only: touches no device, works with no GPU present. */
int plk_msm_plan(size_t n, int batch, int aligned, int out[5]);
int plk_msm_g1_serial_dev(const uint8_t *d_points, const uint8_t *d_scalars, size_t n,
                          plk_msm_result_t *d_res, void *stream);
/* out3 = EXP[(sum of count partial logs) mod 102] -- combines per-shard partials after a
 * collective sum (multi-GPU point-range sharding). */
int plk_msm_combine_dev(const uint32_t *d_logs, int count, uint8_t *d_out3, void *stream);
/* batch of already-summed logs (element i at d_logs[i * stride]) -> d_out4[4 i ..] =
 * {x, y, infinite, 0} of EXP[log mod 102]; one launch for a whole batch of MSMs. */
int plk_msm_finalize_dev(const uint32_t *d_logs, int batch, int stride, uint8_t *d_out4,
                         void *stream);
/* the order-102 generator the logs refer to (the first affine point of order 102 in (x, y)
 * order) */
int plk_dlog_generator(uint8_t out[3]);

/* ---- Segmented MSM: a ragged list of MSMs in one call, flat 4-byte results ------------------
 * Very many small or uneven sums over arbitrary points, with results the next call can read as they
 * stand: the weighted sum of the commitments of a fold or multi-point job, the proofs of many provers
 * combined in groups of different sizes.  One call takes any list of nseg consecutive segments of ONE
 * flat point array (3 total bytes) and scalar array (total bytes) and returns one 4-byte word per segment.
 *
 * Segments.  Segment g is points and scalars [o_g, o_{g+1}).
 *   uniform (d_offsets == NULL): o_g = g m; m >= 1 and total == m nseg.
 *   ragged  (d_offsets != NULL): o_g = d_offsets[g], nseg + 1 words; m is ignored.  The offsets should
 *           rise (not necessarily strictly) from any o_0 >= 0 to o_nseg <= total; bytes outside the
 *           segments are not looked at for the results; an empty segment is legal.
 * Results.  With status 0, d_out4[4 g ..] = {x, y, infinite, 0} are exactly the three bytes
 *   plk_msm_g1(points + 3 o_g, scalars + o_g, o_{g+1} - o_g) returns: the reference's srs_eval_at_s fold
 *   (src/srs.h:53-68), for ANY scalar byte (g1_mul takes the raw byte).  An empty segment gives the
 *   identity {0, 0, 1}.
 *   _dev form (asynchronous on `stream`): a segment holding a point that is not a canonical group element
 *   in the MSM's sense ({0, 0, 1} or an on-curve affine point with flag 0) gets status
 *   PLK_MSM_SEG_IRREGULAR and the bytes FF FF FF, which the verify calls answer with 2; a bad point flags
 *   the segment that holds it and no other.  In ragged form every offset is read as min(o, total); a
 *   segment with o_{g+1} < o_g or with an offset above total gets PLK_MSM_SEG_BAD and FF FF FF.  No offset
 *   value whatever makes a kernel read outside [0, total) of the two arrays or outside the nseg + 1
 *   offset words, and neighbours are unaffected.
 *   Host form (synchronous): the offsets are validated on the host (a falling offset or one above total
 *   is PLK_ERR_ARG before any device query) and irregular segments are resolved exactly with the
 *   library's raw serial fold, as plk_msm_g1 does: the call is exact for every input byte and out3 (3
 *   bytes per segment) needs no status.
 * Geometry depends on (total, m, nseg, ragged) only.  plk_msm_g1_segments_plan (host only, no device
 * touched) reports it:
 *   out[0]  path: 0 lane (uniform, m <= 32: one lane per segment, one launch), 1 prefix (everything else:
 *           a streaming pass over the POINT range stores scanned partial sums, a one-block scan of the
 *           tile totals, then one lane per segment: at most 32 points summed from their bytes, a longer
 *           segment as a difference of two prefixes)
 *   out[1]  points per block tile of the first launch
 *   out[2]  launches: 1 or 3
 *   out[3]  blocks of the first launch
 * The ragged form runs the streaming pass even when every segment is short: the library cannot know the
 * lengths without reading device memory.
 * d_work: plk_msm_g1_segments_workspace bytes (4 per 16 points + 8 per tile), 4-byte aligned, 0 exactly
 * where the plan says one launch, and d_work may then be NULL.  Neither d_work nor d_out4 needs
 * initialisation: every word read was written by the same call, no atomics are used, a workspace may be
 * reused by the next call on the stream, and calls on different streams with distinct workspaces may run
 * concurrently.  Results are bit-identical from run to run.  Exactly 4 nseg bytes of d_out4 are written.
 * Points, scalars and out may have any alignment (offsets 4 bytes); 16-byte aligned points and scalars
 * take vector loads, with the same result.
 * Errors (all before any device query): a NULL pointer (d_work only where the workspace is not 0),
 * nseg == 0, total == 0, or uniform with m == 0 or m nseg != total are PLK_ERR_ARG; total >= 2^32 or
 * nseg > 2^30 is PLK_ERR_RANGE; the plan returns the same codes for its arguments and the workspace
 * function 0.  No GPU is PLK_ERR_NODEV -- there is no CPU fallback.  The device rules are those of
 * plk_kzg_verify_batch(_dev). */
#define PLK_MSM_SEG_IRREGULAR 1   /* status: some encoding of the segment is not a canonical group element */
#define PLK_MSM_SEG_BAD       2   /* status (_dev, ragged only): o[g+1] < o[g] or o[g+1] > total */
int    plk_msm_g1_segments_plan(size_t total, size_t m, size_t nseg, int ragged, int64_t out[4]);  /* host only */
size_t plk_msm_g1_segments_workspace(size_t total, size_t m, size_t nseg, int ragged);             /* host only; 0: bad args or none needed */
int plk_msm_g1_segments_dev(const uint8_t *d_points /* 3 total */, const uint8_t *d_scalars /* total */, size_t total,
                            const uint32_t *d_offsets /* DEVICE, nseg + 1 words, or NULL */, size_t m, size_t nseg,
                            uint8_t *d_out4 /* 4 nseg */, void *d_work, void *stream);
int plk_msm_g1_segments(const uint8_t *points, const uint8_t *scalars, size_t total,
                        const uint32_t *offsets /* host, or NULL */, size_t m, size_t nseg, uint8_t *out3 /* 3 nseg */);

/* poly_mul on device buffers: d_out holds la+lb-1 bytes (not overlapping d_a / d_b); *d_out_nz
 * receives the trimmed length (0 = the zero polynomial, i.e. length 1).  d_work:
 * plk_poly_mul_workspace() bytes.  d_a, d_b and d_out may have any alignment; exactly la and lb
 * bytes are read, exactly la+lb-1 bytes of d_out, the one word at d_out_nz and at most
 * plk_poly_mul_workspace() bytes of d_work are written, whatever lies beside them (no kernel
 * choice of poly_mul depends on an address). */
size_t plk_poly_mul_workspace(size_t la, size_t lb);
int plk_poly_mul_dev(const uint8_t *d_a, size_t la, const uint8_t *d_b, size_t lb, uint8_t *d_out,
                     uint32_t *d_out_nz, void *d_work, void *stream);

/* A batch of independent poly_mul products on device buffers (the prover's round-3 products
 * run this way; replaces a sequence of poly_mul calls, src/poly.h:106-122): products of one
 * transform size share each pass's launch, and operands given by the same pointer and length
 * are transformed once.  acc = 1 ADDS the product into the preceding job's output (a sum group:
 * a leader and up to two members of its transform size, none with a longer product than the
 * leader's; the members' out is not written; the whole sum must fit the transform's exact
 * range, else PLK_ERR_RANGE).  Outputs are
 * untrimmed (la + lb - 1 bytes) and must not overlap any job's inputs (the last pass still reads
 * input bytes for the top coefficients of wrapped products).  d_work: at least the largest single
 * job's plk_poly_mul_workspace() (a sum group of g products: g times its member's); products run
 * in launches of up to 12, cut between sum groups; plk_poly_mul_batch_workspace() bytes run every
 * size group at full width.  Every a, b and out may have any alignment; exactly la and lb bytes of
 * each operand are read, exactly la + lb - 1 bytes of each non-member out and at most work_bytes of
 * d_work are written. */
typedef struct {
  const uint8_t *a;
  size_t la;
  const uint8_t *b;
  size_t lb;
  uint8_t *out;
  int acc;
} plk_polymul_job_t;
size_t plk_poly_mul_batch_workspace(const plk_polymul_job_t *jobs, int n);
int plk_poly_mul_batch_dev(const plk_polymul_job_t *jobs, int n, void *d_work, size_t work_bytes, void *stream);

/* Radix-2 NTT over BabyBear p = 15*2^27+1 on 2^log_n Montgomery-form u32, in place:
 * forward = DIF natural -> bit-reversed; inverse = DIT bit-reversed -> natural, unscaled. */
int plk_ntt_dev(uint32_t *d_data, int log_n, int inverse, void *stream);
/* batch independent transforms of 2^log_n points, array b at d_data + b 2^log_n; the arrays
 * share each pass's launch (the prover's products run the same way). */
int plk_ntt_batch_dev(uint32_t *d_data, int log_n, int batch, int inverse, void *stream);
/* The same over F29 p = 7*2^26+1 -- the field poly_mul and the device prover transform in
 * (lazy reduction inside, ~7 integer VALU per butterfly against ~10 for BabyBear): Montgomery
 * form (R = 2^32) u32 < p in, fully reduced out, root of order 2^log_n = 3^((p-1)/2^log_n);
 * log_n 13..26. */
int plk_ntt29_dev(uint32_t *d_data, int log_n, int inverse, void *stream);
int plk_ntt29_batch_dev(uint32_t *d_data, int log_n, int batch, int inverse, void *stream);

/* ---- the ops around the hot path ---------------------------------
 * Byte-exact restatements of the reference's host ops on the GPU, for every byte value
 * (non-canonical HF bytes included: the kernels fall back to the reference's serial loop on the
 * device where the parallel form would differ).  The drop-in headers call them. */

/* Replaces poly_eval (src/poly.h:265-272): Horner at x, *y = the reference's HF byte. */
int plk_poly_eval(const uint8_t *p, size_t len, uint8_t x, uint8_t *y);
/* n evaluations in one launch (the prover's ~40 evaluations, src/plonk.h:345-347, 527-533,
 * 567, 574; the grand-product loop src/plonk.h:326-359): ys[i] = poly_eval(polys[i], xs[i]). */
int plk_poly_eval_batch(const uint8_t *const *polys, const size_t *lens, const uint8_t *xs, int n,
                        uint8_t *ys);
/* device form: d_polys = host array of n device pointers; d_tick = plk_poly_eval_workspace(n)
 * bytes of device memory, zeroed once (every launch leaves it zeroed again). */
size_t plk_poly_eval_workspace(int n);
int plk_poly_eval_batch_dev(const uint8_t *const *d_polys, const size_t *lens, const uint8_t *xs, int n,
                            uint8_t *d_ys, void *d_tick, void *stream);

/* Replaces poly_divide (src/poly.h:124-177): num = quot * den + rem.
 *   quot: max(nl - dl + 1, 1) bytes, rem: min(dl - 1, nl) bytes (may be NULL when that is 0);
 *   *quot_len / *rem_len = lengths after the reference's trim (rem_len 0 when dl == 1).
 * Divisors x^m * lead + d0 (Z_H = x^n - 1, x - z, constants) run as parallel chain scans; any
 * other canonical divisor of at least PLK_OPT_DIVIDE_FAST_MIN loop steps runs as a Newton inverse
 * over exact poly_mul products (byte-identical: Euclidean division over GF(17) is unique); smaller
 * ones, non-canonical divisors and non-canonical numerator bytes run the reference's loop on the
 * device (one thread).
 * A zero divisor is PLK_ERR_ARG ("Division by zero polynomial in poly_divide"); a divisor lead
 * byte >= 17 is PLK_ERR_RANGE (the reference reads hf_inverses out of bounds). */
int plk_poly_divide(const uint8_t *num, size_t nl, const uint8_t *den, size_t dl, uint8_t *quot, size_t *quot_len,
                    uint8_t *rem, size_t *rem_len);
/* device form: den stays a HOST array (classified on the host, copied into d_work when the
 * serial loop needs it); d_lens[0..1] receive the index + 1 of the last non-zero quotient /
 * remainder byte (0: all zero) over the untrimmed lengths above; d_work:
 * plk_poly_divide_workspace(nl, dl) bytes (sized for the Newton path of every shape that could take
 * it, whatever PLK_OPT_DIVIDE_FAST_MIN is; it does depend on PLK_OPT_POLY_BLOCK_L / _S as
 * plk_poly_mul_workspace does). */
size_t plk_poly_divide_workspace(size_t nl, size_t dl);
int plk_poly_divide_dev(const uint8_t *d_num, size_t nl, const uint8_t *den, size_t dl, uint8_t *d_quot,
                        uint8_t *d_rem, uint32_t *d_lens, void *d_work, void *stream);
/* The path plk_poly_divide / plk_poly_divide_dev take for this divisor (a HOST array) and numerator
 * length under the current options: 0 trivial (nl < dl), 1 constant, 2 binomial chain scans, 3 the
 * reference's loop on one thread, 4 Newton inverse.  A zero divisor gives -PLK_ERR_ARG, a lead
 * byte >= 17 -PLK_ERR_RANGE.  Host only: touches no device, works with no GPU present. */
int plk_poly_divide_path(const uint8_t *den, size_t dl, size_t nl);

/* Replaces matrix_mul (src/matrix.h:79-96): out[m x n] = a[m x k] b[k x n], row-major bytes,
 * sums by hf_add of hf_mul products. */
int plk_matrix_mul(const uint8_t *a, size_t m, size_t k, const uint8_t *b, size_t n, uint8_t *out);
/* Replaces matrix_inv (src/matrix.h:149-176, Gauss-Jordan src/matrix.h:100-147) as plonk_new
 * uses it for the Vandermonde inverse h_pows_inv (src/plonk.h:105-113): the same pivoting, so
 * the same bytes for singular matrices too.  Entries must be GF(17) values (< 17). */
int plk_matrix_inv(const uint8_t *mat, size_t n, uint8_t *out);
/* interpolate_at_h (src/plonk.h:162-195): out = h_pows_inv (n x n) * values, trimmed as
 * poly_new; out holds n bytes. */
int plk_interpolate(const uint8_t *h_pows_inv, const uint8_t *values, size_t n, uint8_t *out, size_t *out_len);

/* ---- poly linear combinations: add, sub, scale, negate, shift, twist in one pass ---------
 * The reference's elementwise polynomial ops (src/poly.h:66-104, 179-216, 240-254: poly_add_hf, poly_add,
 * poly_sub, poly_scale, poly_shift, poly_negate; poly_slice is p + start, end - start) and the x -> omega x
 * coefficient loop of src/plonk.h:466-470, composed over up to PLK_LC_MAX_TERMS polynomials in one pass
 * over device buffers: with these the _dev entry points are closed under the operations of a KZG / PLONK
 * round (tests/test_public_api_prove_gpu.py rebuilds a whole proof from them).
 *
 * Semantics (the specification).  Each term is transformed in the order twist -> scale -> negate -> shift;
 * the accumulator starts as term 0 transformed; every later term is folded in, in order, with the
 * reference's poly_add or poly_sub; poly_add_hf is applied last, to coefficient 0.  Per coefficient j < L
 * = max_i(len_i + shift_i): the byte formulas are the reference's own hf_add, hf_sub, hf_neg, hf_mul with
 * their uint8_t / int8_t behaviour on bytes >= 17; a term contributes hf_zero() outside
 * [shift, shift + len) and the operation is still applied there (as poly_add does for i >= len).  The
 * reference trims intermediate results; those trims change no byte (past a trimmed length both operands
 * read as zero), so out is the untrimmed result over L bytes, exact for EVERY input byte value.
 * d_nz[b] receives the index + 1 of the last non-zero byte of job b (0: all zero) -- the convention of
 * plk_poly_mul_dev -- and needs no initialisation by the caller.
 * Aliasing: out may be exactly a term's p when that term's shift is 0 (accumulation in place).  Any other
 * overlap of an output with any job's input, or with another output, of the same call is the caller's
 * error.
 * Batch: any n; a launch carries whole jobs up to a fixed number of jobs and terms, larger batches run as
 * consecutive launches on the stream.  The call needs no workspace and keeps no state; pointers may have
 * any alignment (16-byte aligned ones run fastest).  Calls on different streams may run concurrently.
 * Errors (all checked before any device query): a NULL pointer, n <= 0, nterms outside
 * 1 .. PLK_LC_MAX_TERMS, len == 0, sub or neg > 1, scale in 17 .. 254, twist > 16, add_hf outside -1 .. 16
 * or term 0 with sub = 1 are PLK_ERR_ARG; L >= 2^32 is PLK_ERR_RANGE.  No GPU is PLK_ERR_NODEV -- there is
 * no CPU fallback.  The device rules are those of plk_kzg_verify_batch(_dev). */
#define PLK_LC_MAX_TERMS 16
#define PLK_LC_RAW 0xFF
typedef struct {
  const uint8_t *p;   /* coefficients (device pointer in the _dev form) */
  size_t len;         /* >= 1 */
  size_t shift;       /* poly_shift: coefficient i lands at i + shift */
  uint8_t sub;        /* 0: folded in with poly_add, 1: with poly_sub (term 0: must be 0) */
  uint8_t scale;      /* 0..16: poly_scale by it (hf_mul per byte; 0 gives poly_zero);
                         PLK_LC_RAW: the bytes as they are */
  uint8_t neg;        /* 1: poly_negate (hf_neg per byte) */
  uint8_t twist;      /* 0: none; 1..16: coefficient i becomes hf_mul(p[i], hf_pow(twist, i)),
                         the x -> twist*x substitution of src/plonk.h:466-470 */
} plk_lc_term_t;
typedef struct {
  const plk_lc_term_t *terms;   /* HOST array, 1..PLK_LC_MAX_TERMS */
  int nterms;
  int add_hf;                   /* -1: none; 0..16: poly_add_hf(result, add_hf) at the end */
  uint8_t *out;                 /* L = max_i(len_i + shift_i) bytes, every one written */
} plk_lc_job_t;
size_t plk_poly_lincomb_len(const plk_lc_job_t *job);            /* L; host only; 0 for bad arguments */
int plk_poly_lincomb(const plk_lc_job_t *job, size_t *out_len);  /* host buffers, synchronous;
                                                                    *out_len trimmed as poly_new, >= 1 */
int plk_poly_lincomb_batch_dev(const plk_lc_job_t *jobs, int n, uint32_t *d_nz /* n words or NULL */,
                               void *stream);

/* ---- division by short divisors: a ragged batch, one streaming scan each -----------------
 * poly_divide (src/poly.h:124-177) of device polynomials by divisors of 2 .. PLK_DIV_SHORT_MAX coefficients
 * (degree t = dl - 1 in 1 .. 16: x - z, (x - z)(x - z omega), a vanishing polynomial Z_S of a small point
 * set, the dense Z_H of n <= 16), a whole batch per call.  Division by such a divisor is a t-state linear
 * recurrence over the numerator from its top coefficient down; it runs as one scan whose traffic is two
 * reads and one write of the numerator.  plk_poly_divide(_dev) and their routing are
 * unchanged and do not use this path.
 *
 * Semantics (the specification).  For every numerator whose bytes are all < 17, job b's quot bytes, rem
 * bytes and trimmed lengths equal those of plk_poly_divide(num, nl, den, dl, ...), nl < dl included (q =
 * {0}, rem = num).  The outputs are untrimmed: max(nl - dl + 1, 1) quotient bytes and min(dl - 1, nl)
 * remainder bytes, every one written.  d_lens[3b] and d_lens[3b + 1] receive the index + 1 of the last
 * non-zero quotient and remainder byte (0: all zero), d_lens[3b + 2] is 0, or 1 when the numerator holds a
 * byte >= 17.  _dev form: a job with status 1 has unspecified bytes inside its own quot and rem buffers and
 * unspecified length words; its neighbours are unaffected.  Host form: such a job runs through
 * plk_poly_divide, so the call is exact for every numerator byte (the convention of plk_kzg_open_batch);
 * quot_lens / rem_lens are trimmed as plk_poly_divide returns them (>= 1).
 * d_work: plk_poly_divide_short_workspace(jobs, n) bytes; neither it nor d_lens needs initialisation, and
 * a workspace may be reused by the next call on the same stream.  den is a HOST array and is not referenced
 * after the call returns.  Any n: the jobs run grouped by divisor length class (dl <= 3, <= 5, <= 9, <= 17),
 * PLK_DIV_SHORT_LAUNCH_JOBS jobs to a group; a group is one kernel when every job of it fits one block's
 * span and three otherwise, one memset node in front of the call's launches.  Pointers may have any
 * alignment (d_lens: 4 bytes).  An output may overlap no input and no other output of the call.  Calls on
 * different streams with distinct workspaces may run concurrently.
 * Errors (all raised before any device query): a NULL pointer, n <= 0, nl == 0, dl < 2, a divisor byte >= 17
 * or a zero lead are PLK_ERR_ARG; dl > PLK_DIV_SHORT_MAX or nl >= 2^32 is PLK_ERR_RANGE.  No GPU is
 * PLK_ERR_NODEV.  The device rules are those of plk_kzg_verify_batch(_dev).
 * plk_poly_divide_short_plan (host only) fills out[] for one job of shape (nl, dl) run alone: {kernels (1 or
 * 3), coefficients per thread, coefficients per block, the largest nl of this dl that runs as one kernel};
 * it returns PLK_ERR_ARG / PLK_ERR_RANGE as the launch would.
 * plk_poly_from_roots (host only) writes the t + 1 coefficients of prod (x - roots[i]), t in 1 .. 16, roots
 * < 17, repeats allowed (PLK_ERR_ARG: NULL, t < 1, a root >= 17; PLK_ERR_RANGE: t > 16): the Z_S of a
 * point set. */
#define PLK_DIV_SHORT_MAX 17          /* divisor coefficients: degree 1..16 */
#define PLK_DIV_SHORT_LAUNCH_JOBS 32  /* jobs a group of launches carries */
typedef struct {
  const uint8_t *num; size_t nl;  /* device pointer in the _dev form; nl >= 1 */
  const uint8_t *den; size_t dl;  /* HOST array, 2..PLK_DIV_SHORT_MAX bytes, all < 17, den[dl-1] != 0 */
  uint8_t *quot;                  /* max(nl - dl + 1, 1) bytes, every one written */
  uint8_t *rem;                   /* min(dl - 1, nl) bytes, every one written */
} plk_divshort_job_t;
size_t plk_poly_divide_short_workspace(const plk_divshort_job_t *jobs, int n); /* host only; 0: bad args */
int plk_poly_divide_short_plan(size_t nl, size_t dl, int out[4]);              /* host only */
int plk_poly_divide_short_batch_dev(const plk_divshort_job_t *jobs, int n,
                                    uint32_t *d_lens /* 3 n words */, void *d_work, void *stream);
int plk_poly_divide_short_batch(const plk_divshort_job_t *jobs, int n,
                                size_t *quot_lens, size_t *rem_lens);          /* host buffers, synchronous */
int plk_poly_from_roots(const uint8_t *roots, int t, uint8_t *out /* t + 1 */); /* host only */

/* ---- products by short operands: whole runs of equal-shape products in one launch -------
 * poly_mul (src/poly.h:106-122) of device polynomials where the shorter operand has at most
 * PLK_MUL_SHORT_MAX coefficients: the many small products of small circuits, and long polynomials times a
 * blinding polynomial, a Z_S from plk_poly_from_roots or a selector of a few hundred coefficients.  The
 * products run as a schoolbook convolution over packed bytes, any number of them per
 * launch.  plk_poly_mul, plk_poly_mul_dev, plk_poly_mul_batch_dev and their routing are unchanged and do not
 * use this path.
 *
 * A run is count products of one shape at fixed strides: product i reads la bytes at a + i * a_stride and lb
 * bytes at b + i * b_stride and writes la + lb - 1 bytes at out + i * out_stride.  A ragged batch is a list of
 * runs with count = 1.  Any stride may be 0 (a shared operand) or smaller than the operand (overlapping
 * reads).  The run array is a HOST array and is not referenced after the call returns.
 *
 * Semantics (the specification).  Product i of run r writes exactly the la + lb - 1 untrimmed bytes that
 * plk_poly_mul(a_i, la, b_i, lb, ...) produces, for EVERY input byte value: hf_mul reduces each product and
 * hf_add keeps the sum canonical (src/hf.h:79-109), so the result is conv(a mod 17, b mod 17) mod 17.  Bytes
 * between consecutive outputs (out_stride > la + lb - 1) are not written.  d_nz may be NULL; otherwise it
 * holds one word per product in run order (product i of run r at count_0 + ... + count_{r-1} + i), each
 * receiving the index + 1 of the last non-zero output byte (0: all zero) -- the convention of
 * plk_poly_mul_dev -- and needs no initialisation by the caller (one memset node in front of the launches).
 * Host form: synchronous, staged through device buffers on the primary device; out_lens (one entry per
 * product, may be NULL) is trimmed as plk_poly_mul returns it (>= 1).
 * Batch: any n; a launch carries PLK_MUL_SHORT_LAUNCH_RUNS whole runs, larger batches run as consecutive
 * launches on the stream.  No workspace, no state; pointers may have any alignment (d_nz: 4 bytes).  An
 * output may overlap no input and no other output of the call.  Calls on different streams may run
 * concurrently.
 * Errors (all raised before any device query): a NULL runs, a, b or out, n <= 0, count == 0, la == 0,
 * lb == 0, or count > 1 with out_stride < la + lb - 1 are PLK_ERR_ARG; min(la, lb) > PLK_MUL_SHORT_MAX,
 * la + lb - 1 >= 2^32, more than 2^24 products in one call, or a run that alone needs more blocks than a
 * grid holds are PLK_ERR_RANGE.  No GPU is PLK_ERR_NODEV -- there is no CPU fallback.  The device rules are
 * those of plk_kzg_verify_batch(_dev).
 * plk_poly_mul_short_plan (host only) fills out[] for one run of count products of shape (la, lb) alone:
 * {outputs per work unit, work units per product, work units per block, blocks}; it returns the error the
 * launch would return. */
#define PLK_MUL_SHORT_MAX 1024          /* coefficients of the shorter operand */
#define PLK_MUL_SHORT_LAUNCH_RUNS 32    /* whole runs a launch carries */
typedef struct {
  const uint8_t *a; size_t la; size_t a_stride;   /* product i reads la bytes at a + i * a_stride   */
  const uint8_t *b; size_t lb; size_t b_stride;   /* ... and lb bytes at b + i * b_stride           */
  uint8_t *out;     size_t out_stride;            /* writes la + lb - 1 bytes at out + i * out_stride */
  size_t count;                                   /* >= 1 products of this one shape                 */
} plk_mulshort_run_t;                             /* pointers: device in the _dev form, host in the host form */
int plk_poly_mul_short_plan(size_t la, size_t lb, size_t count, int64_t out[4]);           /* host only */
int plk_poly_mul_short_batch_dev(const plk_mulshort_run_t *runs, int n, uint32_t *d_nz, void *stream);
int plk_poly_mul_short_batch(const plk_mulshort_run_t *runs, int n, size_t *out_lens);

/* ---- KZG over a resident SRS: commit and open, batched ----------------------------------
 * The commitment (srs_eval_at_s, src/srs.h:53-68) and the opening the reference spells out twice per
 * proof (src/plonk.h:606-621: y = p(z), q = (p - y) / (x - z), [q]) against an SRS that stays on the
 * device.  plk_srs_create uploads len G1s (3 B each) to the current device -- which must be the
 * library's primary device -- and keeps the G1 form and, when every encoding is a canonical group
 * element, the log form (1 B per point) the fast path reads.  The handle is immutable after
 * creation and holds the library context like a prover (plk_shutdown keeps the tables while one is
 * alive); every call on it is made with the handle's device current (PLK_ERR_ARG otherwise).
 *
 * Semantics (the specification; job b of a batch of n, any n):
 *   commit  = plk_msm_g1(srs[0 .. lens[b]), polys[b], lens[b]) exactly, for any coefficient byte
 *             (g1_mul takes the raw byte).
 *   open    = the composition  y = plk_poly_eval(p, len, z);
 *             (q, q_len) = the quotient of plk_poly_divide(p, len, {(17 - z) % 17, 1}, 2);
 *             proof = plk_msm_g1(srs, q, q_len)      (len == 1: q = {0}, proof = the identity).
 * The fast path serves the canonical case, every coefficient < 17 and a regular SRS: a ragged batch
 * of commitments is one launch; a batch of openings is two (per-chunk aggregates of the suffix scan,
 * then quotient bytes in registers dotted with the SRS logs; one when every polynomial has at most
 * 4096 coefficients), and the quotient is stored only where asked for.  Launches carry 32 jobs
 * each; larger batches run in consecutive launches on the stream.
 *   Host forms (synchronous): a job with a coefficient byte >= 17, and every job when
 *   plk_srs_irregular, runs that composition itself, its commitment over the resident G1 form (the
 *   dlog launch, then the raw serial fold when that says irregular, as plk_msm_g1 does).
 *   _dev forms (asynchronous; d_polys / d_quots are HOST arrays of device pointers, lens and zs host
 *   arrays): such a job is left with d_res[b].irregular > 0 and g1 invalid -- the convention of
 *   plk_msm_g1_dev -- while its batch neighbours are unaffected.  d_ys[b] and the bytes at
 *   d_quots[b] (max(len - 1, 1) of them, untrimmed) are exact whenever the coefficients are
 *   canonical, whatever the SRS.  Records: zeroed once (plk_msm_result_init), then reusable.
 *   d_work: plk_kzg_workspace(lens, n) bytes, no initialisation needed (every word read was written
 *   by the same call); may be NULL when no polynomial has more than 4096 coefficients.  Calls on
 *   different streams with distinct workspaces and records may run concurrently.
 * Errors: a NULL handle or array, n <= 0, lens[b] == 0, zs[b] >= 17 or a call from another device
 * are PLK_ERR_ARG (checked before any device query); commit with lens[b] > plk_srs_len and open with
 * max(lens[b] - 1, 1) > plk_srs_len are PLK_ERR_RANGE on the lengths as given (the reference's
 * "degree exceeds SRS size": its callers pass trimmed polynomials); plk_srs_create with no GPU is
 * PLK_ERR_NODEV. */
typedef struct plk_srs plk_srs_t;
int plk_srs_create(const uint8_t *g1s, size_t len, plk_srs_t **out);
void plk_srs_destroy(plk_srs_t *s);              /* NULL: no-op */
size_t plk_srs_len(const plk_srs_t *s);          /* 0 for NULL */
int plk_srs_irregular(const plk_srs_t *s);       /* 1: some encoding is not a canonical group element */
int plk_kzg_commit_batch(const plk_srs_t *s, const uint8_t *const *polys, const size_t *lens, int n,
                         uint8_t *out3 /* 3 n */);
int plk_kzg_open_batch(const plk_srs_t *s, const uint8_t *const *polys, const size_t *lens,
                       const uint8_t *zs, int n, uint8_t *ys /* n */, uint8_t *proofs3 /* 3 n */);
size_t plk_kzg_workspace(const size_t *lens, int n);   /* host only, no device touched; 0 for bad arguments */
int plk_kzg_commit_batch_dev(const plk_srs_t *s, const uint8_t *const *d_polys, const size_t *lens, int n,
                             plk_msm_result_t *d_res, void *stream);
int plk_kzg_open_batch_dev(const plk_srs_t *s, const uint8_t *const *d_polys, const size_t *lens,
                           const uint8_t *zs, int n, uint8_t *d_ys, plk_msm_result_t *d_res,
                           uint8_t *const *d_quots /* NULL, or per job NULL / max(len-1,1) bytes */,
                           void *d_work, void *stream);

/* ---- Pairings and KZG verification: batched, one lane per job ----------------------------
 * The reference's pairing() (src/pairing.h:66-83) over n independent (G1, G2) pairs in one launch,
 * and the check of a KZG opening (C, z, y, W) built from it.  All group arithmetic of the check is
 * in G1 (the reference's G2 has no identity encoding, which sH - zH would need at z = s):
 *     L  = C - y G + z W                        G = [1]_1, W = the proof
 *     ok = pairing(L, [1]_2) == pairing(W, [s]_2)
 * Only KZG openings are verified.  No verifier of the reference's PLONK proofs is offered, because
 * none can be sound: plonk_prove's linearisation contains a product of two committed polynomials
 * (src/plonk.h:557-564), so a verifier cannot form [r]_1 from the commitments.
 *
 * Encodings: G1 3 bytes {x, y, infinite} as everywhere; G2 2 bytes {x, y} (src/g2.h:7-9); GT 2 bytes
 * {a, b} = a + b u with u^2 = -2 (src/gt.h:7-9).  Valid: G1 x, y < 101 and flag 0 or 1 -- on the
 * curve or off it, and an identity flag with non-zero coordinates is allowed; G2 x, y < 101;
 * z, y < 17.
 *
 * Semantics (the specification; job b of a batch of n):
 *   pairing  a valid pair gives the reference's pairing() bytes exactly.  The reference applies its
 *            formulas blindly and so does the kernel: no curve-membership test, no subgroup test.
 *            An invalid pair gives {0xFF, 0xFF}; its batch neighbours are unaffected.
 *   verify   ok[b] = gtp_equal(pairing(&L, &vk->g2_1), pairing(&W, &vk->g2_s)), 1 or 0, with
 *                yG = g1_mul(&G, y); nyG = g1_neg(&yG); zW = g1_mul(&W, z);
 *                L = g1_add(&C, &nyG); L = g1_add(&L, &zW);         (G = vk->g1)
 *            A job with an invalid byte in C, W, z or y gets ok[b] = 2; its neighbours are unaffected.
 * The verification key is 7 bytes read at the call: no handle, not tied to plk_srs_t (a verifier
 * never holds the SRS).  Host forms are synchronous and run on the library's primary device, which
 * they make the calling thread's current device as the other host-buffer entry points do.  _dev forms
 * are asynchronous on `stream`, need no workspace, keep no state and use no atomics; their pointers
 * may have any alignment; the calling thread's current device must be the library's (the pointers and
 * the stream belong to it).
 * Errors: a NULL pointer, n == 0 or an invalid byte in vk are PLK_ERR_ARG, n > 2^30 is PLK_ERR_RANGE
 * (both before any device query); no GPU is PLK_ERR_NODEV -- there is no CPU fallback; a _dev call
 * from a thread whose current device is not the library's is PLK_ERR_ARG. */
typedef struct { uint8_t g1[3]; uint8_t g2_1[2]; uint8_t g2_s[2]; uint8_t pad; } plk_kzg_vk_t;  /* 8 bytes: [1]_1, [1]_2, [s]_2 */
int plk_pairing_batch(const uint8_t *g1s /* 3 n */, const uint8_t *g2s /* 2 n */, size_t n, uint8_t *out_gt /* 2 n */);
int plk_pairing_batch_dev(const uint8_t *d_g1s, const uint8_t *d_g2s, size_t n, uint8_t *d_out_gt, void *stream);
int plk_kzg_verify_batch(const plk_kzg_vk_t *vk, const uint8_t *commits3, const uint8_t *zs, const uint8_t *ys,
                         const uint8_t *proofs3, size_t n, uint8_t *ok /* n */);
int plk_kzg_verify_batch_dev(const plk_kzg_vk_t *vk /* HOST */, const uint8_t *d_commits3, const uint8_t *d_zs,
                             const uint8_t *d_ys, const uint8_t *d_proofs3, size_t n, uint8_t *d_ok, void *stream);

/* ---- KZG folded openings: k polynomials at one point, one proof ---------------------------
 * The form KZG-based protocols use (the reference's plonk_prove round 5, src/plonk.h:582-621):
 * polynomials p_0 .. p_{k-1} opened at the same z under caller-chosen weights w_i with ONE proof, the
 * commitment of (sum_i w_i (p_i - p_i(z))) / (x - z), and that proof verified against the k
 * commitments with two pairings.
 *
 * Opening.  The polynomials of a call lie in flat arrays; group g = entries [start[g], start[g+1]),
 * start[0] = 0, strictly increasing, 1 .. PLK_KZG_FOLD_MAX entries a group, ngroups >= 1,
 * npolys = start[ngroups].  For group g with L = the largest of its lens and z = zs[g] (the
 * specification):
 *   ys[i]      = plk_poly_eval(p_i, lens[i], z)                    for every polynomial of the group
 *   F[j]       = the hf_add fold over i of hf_mul(w_i, p_i[j]), j < L, a polynomial contributing
 *                nothing past its own length (the reference's poly_scale / poly_add without the trim;
 *                hf_mul reduces, so F depends on the bytes mod 17 only and is always canonical)
 *   proofs3[g] = the proof plk_kzg_open_batch gives for (F, L, z) -- which covers all weights zero,
 *                F cancelling to a shorter degree or to zero, L = 1, and an irregular SRS
 *   d_quots[g] = max(L - 1, 1) untrimmed bytes of (F - F(z)) / (x - z), exact for EVERY coefficient
 *                byte and any SRS (F is canonical whatever the input bytes)
 * The fast path is one fused pass: F is formed in registers (sum_i w_i x byte is exact in 16 bits,
 * one reduction per coefficient) and handed to the opening kernel's suffix scan; an aggregates launch
 * in front of it when some L > 4096.  A launch carries whole groups, up to 32 polynomials; larger
 * batches run in consecutive launches on the stream.
 *   Host form (synchronous): a group holding a coefficient byte >= 17, and every group when
 *   plk_srs_irregular, returns the composition's bytes: its ys through plk_poly_eval, its proof the
 *   commitment of the (exact) quotient bytes over the resident G1 form, as plk_kzg_open_batch does.
 *   _dev form (asynchronous; d_polys / d_quots HOST arrays of device pointers; lens, weights, start
 *   and zs HOST arrays): a group holding a coefficient byte >= 17 is left with d_res[g].irregular > 0
 *   and g1 invalid (the convention of plk_msm_g1_dev); its d_ys are unspecified, its d_quots still
 *   exact.  With an irregular SRS every record is flagged while ys and quotients stay exact.  Other
 *   groups are unaffected.  Records: zeroed once, then reusable.  d_work:
 *   plk_kzg_fold_workspace(lens, start, ngroups) bytes, no initialisation needed; may be NULL when
 *   every L <= 4096.
 * Errors (all but the last checked before any device query): a NULL handle or array, ngroups <= 0, a
 * start that does not rise strictly from 0, a group of more than PLK_KZG_FOLD_MAX, lens[i] == 0, a
 * weight or z >= 17 or a call from another device are PLK_ERR_ARG; max(L - 1, 1) > plk_srs_len or a
 * length beyond what one record's finish can count is PLK_ERR_RANGE; no GPU is PLK_ERR_NODEV.
 *
 * Verification.  k is uniform over a call (its batches are many tiny jobs, one lane each): job b owns
 * entries [k b, k (b + 1)) of commits3 / weights / ys.  With the reference's raw formulas applied
 * blindly, as plk_kzg_verify_batch applies them (the specification):
 *   acc = g1_identity();  for i in order: term = g1_mul(&C_i, w_i); acc = g1_add(&acc, &term);
 *   y   = the hf_add fold of hf_mul(w_i, y_i) from hf_zero()
 *   ok[b] = the check of plk_kzg_verify_batch on (C = acc, z, y, W)
 * A job with an invalid byte (a G1 coordinate >= 101, a G1 flag > 1, a weight, y or z >= 17) gets
 * ok[b] = 2; its neighbours are unaffected.  k = 1 with w = 1 goes through
 * g1_add(identity, g1_mul(C, 1)), which need not return an off-curve or flagged C byte for byte.
 * Errors: k < 1, k > PLK_KZG_FOLD_MAX, a NULL pointer, n == 0 or an invalid byte in vk are
 * PLK_ERR_ARG, n k > 2^30 is PLK_ERR_RANGE (both before any device query); no GPU is PLK_ERR_NODEV;
 * the device rules are those of plk_kzg_verify_batch(_dev). */
#define PLK_KZG_FOLD_MAX 16   /* polynomials per group */
size_t plk_kzg_fold_workspace(const size_t *lens, const int *start, int ngroups);   /* host only; 0 for bad arguments */
int plk_kzg_open_fold_batch(const plk_srs_t *s, const uint8_t *const *polys, const size_t *lens,
                            const uint8_t *weights /* npolys */, const int *start, const uint8_t *zs /* ngroups */,
                            int ngroups, uint8_t *ys /* npolys */, uint8_t *proofs3 /* 3 ngroups */);
int plk_kzg_open_fold_batch_dev(const plk_srs_t *s, const uint8_t *const *d_polys, const size_t *lens,
                                const uint8_t *weights, const int *start, const uint8_t *zs, int ngroups,
                                uint8_t *d_ys, plk_msm_result_t *d_res /* ngroups */,
                                uint8_t *const *d_quots /* NULL, or per group NULL / max(L-1,1) bytes */,
                                void *d_work, void *stream);
int plk_kzg_verify_fold_batch(const plk_kzg_vk_t *vk, int k, const uint8_t *commits3, const uint8_t *weights,
                              const uint8_t *ys, const uint8_t *zs /* n */, const uint8_t *proofs3 /* 3 n */,
                              size_t n, uint8_t *ok /* n */);
int plk_kzg_verify_fold_batch_dev(const plk_kzg_vk_t *vk /* HOST */, int k, const uint8_t *d_commits3,
                                  const uint8_t *d_weights, const uint8_t *d_ys, const uint8_t *d_zs,
                                  const uint8_t *d_proofs3, size_t n, uint8_t *d_ok, void *stream);

/* ---- KZG multi-point openings: each polynomial at its own point set, two G1s ---------------
 * The second scheme of Boneh-Drake-Fisch-Gabizon over this library's key ([1]_2 and [s]_2 only): a group
 * of k polynomials p_0 .. p_{k-1}, 1 <= k <= PLK_KZG_MULTI_MAX, polynomial i opened at every point of its
 * own set S_i, costs two G1 elements in all and is checked with two pairings.  A set is a uint32_t mask,
 * bit a set <=> a in S_i, bits 0 .. 16 only, 1 .. PLK_KZG_MULTI_POINTS bits set: no repeated points, and
 * the order of the points is ascending.  The weights w_i and the challenge u of a group are the caller's,
 * as everywhere in this library.  With t_i = |S_i|, Z_i = plk_poly_from_roots(S_i ascending), T = the
 * union of the S_i:
 *     q_i = the quotient of p_i by Z_i;   h = sum_i w_i q_i over Lh = max_i max(len_i - t_i, 1) coefficients
 *     c_i = w_i prod_{a in T \ S_i} (u - a);   c_T = prod_{a in T} (u - a)
 *     W   = [h];   W' = the folded opening at u of (p_0 .. p_{k-1}, h) under weights (c_0 .. c_{k-1}, -c_T)
 * sum_i c_i p_i - c_T h takes the value sum_i c_i r_i(u) at u for every u, points of T included (r_i: the
 * remainder of p_i by Z_i), so no choice of u is special.
 *
 * Opening.  Grouping (start), the host / device array conventions, the records ("zeroed once, then
 * reusable"), the device rules and the stream behaviour are those of plk_kzg_open_fold_batch(_dev); sets
 * and weights are flat HOST arrays of npolys entries, us one HOST byte per group.  For group g the library
 * returns exactly the bytes of this sequence of its own host calls (the specification):
 *   ys[17 i + a] = plk_poly_eval(p_i, lens[i], a) for a in S_i, 0xFF elsewhere (all 17 bytes are written)
 *   (q_i, .)     = plk_poly_divide_short_batch of p_i by plk_poly_from_roots(S_i ascending); len_i <= t_i: q_i = {0}
 *   h            = plk_poly_lincomb of the q_i with scale = w_i, folded by poly_add, Lh untrimmed bytes
 *   W            = plk_kzg_commit_batch of h trimmed
 *   c            = plk_kzg_multi_coeffs(sets, weights, k, u)
 *   W'           = the proof plk_kzg_open_fold_batch gives for (p_0 .. p_{k-1}, h untrimmed over Lh), weights c, z = u
 * proofs6[6 g ..] = W then W'; _dev: record 2 g = W, record 2 g + 1 = W'; d_hs[g], where given, receives the
 * Lh untrimmed bytes of h.  The fast path (every coefficient byte < 17, a regular SRS) never forms a q_i:
 * by partial fractions h is a sum over the points a of T of the single-point quotients of
 * sum_{i : a in S_i} (w_i / prod_{b in S_i, b != a} (a - b)) p_i, formed in registers: an
 * aggregates launch when some polynomial has more than 4096 coefficients, one fused launch for ys, h and W
 * (four whole groups per launch, larger batches in consecutive launches), then the folded opening's own
 * launches for W', group by group.
 *   _dev form: a group holding a coefficient byte >= 17 is left with both records irregular > 0 and its
 *   d_ys and h unspecified; with an irregular SRS every record is flagged while ys and h stay exact.  Other
 *   groups are unaffected.  d_work: plk_kzg_multi_workspace(lens, sets, start, ngroups) bytes, always
 *   required (h lives there when d_hs does not ask for it), 4-byte aligned, no initialisation needed.
 *   Host form (synchronous): such groups are recomputed by the sequence above, so the call is exact for
 *   every coefficient byte and any SRS.
 * Errors: a NULL handle or array, ngroups <= 0, a start that does not rise strictly from 0, a group of more
 * than PLK_KZG_MULTI_MAX, lens[i] == 0, a mask that is 0, has a bit above 16 or has all 17 bits set, a weight
 * or u >= 17, or a call from another device are PLK_ERR_ARG (all but the last before any device query);
 * Lh > plk_srs_len, max(max(the longest len_i, Lh) - 1, 1) > plk_srs_len or a length beyond what one record's
 * finish can count are PLK_ERR_RANGE; no GPU is PLK_ERR_NODEV.
 *
 * Verification.  k is uniform over a call; job b owns entries [k b, k (b + 1)) of commits3 / sets / weights,
 * the 17-byte rows [17 k b, 17 k (b + 1)) of ys (only the bytes at points of the set are read), us[b] and
 * proofs6[6 b ..] = W, W'.  With
 *   r_i(u) = sum_{a in S_i} y_ia prod_{b in S_i, b != a} (u - b) / (a - b) mod 17   (Lagrange over S_i)
 *   c      = plk_kzg_multi_coeffs(sets, weights, k, u)
 * ok[b] is the ok byte of plk_kzg_verify_fold_batch with k + 1 entries: commits (C_0 .. C_{k-1}, W), weights
 * c, ys (r_0(u) .. r_{k-1}(u), 0), z = u, proof W' -- the reference's raw formulas applied blindly, as
 * there.  A job with an invalid G1 byte, an invalid mask, a weight or u >= 17, or a y byte >= 17 at a point
 * of its set gets ok[b] = 2; its neighbours are unaffected.  One lane per job, no atomics, no workspace; any
 * alignment except that d_sets is 4-byte aligned.  Errors: those of plk_kzg_verify_fold_batch with k in
 * 1 .. PLK_KZG_MULTI_MAX.
 * plk_kzg_multi_coeffs (host only): c[0 .. k) = c_i, c[k] = (17 - c_T) % 17; PLK_ERR_ARG for a NULL pointer, k
 * outside 1 .. PLK_KZG_MULTI_MAX, an invalid mask, a weight or u >= 17. */
#define PLK_KZG_MULTI_MAX 15      /* polynomials per group: the second proof folds them with h, PLK_KZG_FOLD_MAX in all */
#define PLK_KZG_MULTI_POINTS 16   /* points per set (the divisor stays within PLK_DIV_SHORT_MAX) */
int plk_kzg_multi_coeffs(const uint32_t *sets, const uint8_t *weights, int k, uint8_t u, uint8_t *c /* k + 1 */);
size_t plk_kzg_multi_workspace(const size_t *lens, const uint32_t *sets, const int *start, int ngroups); /* host only; 0: bad args */
int plk_kzg_open_multi_batch(const plk_srs_t *s, const uint8_t *const *polys, const size_t *lens,
                             const uint32_t *sets /* npolys */, const uint8_t *weights /* npolys */,
                             const int *start, const uint8_t *us /* ngroups */, int ngroups,
                             uint8_t *ys /* 17 npolys */, uint8_t *proofs6 /* 6 ngroups: W, W' */);
int plk_kzg_open_multi_batch_dev(const plk_srs_t *s, const uint8_t *const *d_polys, const size_t *lens,
                                 const uint32_t *sets, const uint8_t *weights, const int *start,
                                 const uint8_t *us, int ngroups, uint8_t *d_ys /* 17 npolys */,
                                 plk_msm_result_t *d_res /* 2 ngroups: W at 2g, W' at 2g + 1 */,
                                 uint8_t *const *d_hs /* NULL, or per group NULL / Lh bytes */,
                                 void *d_work, void *stream);
int plk_kzg_verify_multi_batch(const plk_kzg_vk_t *vk, int k, const uint8_t *commits3 /* 3 n k */,
                               const uint32_t *sets /* n k */, const uint8_t *weights /* n k */,
                               const uint8_t *ys /* 17 n k */, const uint8_t *us /* n */,
                               const uint8_t *proofs6 /* 6 n */, size_t n, uint8_t *ok /* n */);
int plk_kzg_verify_multi_batch_dev(const plk_kzg_vk_t *vk /* HOST */, int k, const uint8_t *d_commits3,
                                   const uint32_t *d_sets, const uint8_t *d_weights, const uint8_t *d_ys,
                                   const uint8_t *d_us, const uint8_t *d_proofs6, size_t n, uint8_t *d_ok,
                                   void *stream);

/* ---- KZG aggregate verification: a group of openings, one verdict -----------------------------
 * The form a KZG verifier uses for many openings: a group of m openings (C_i, z_i, y_i, W_i) is checked
 * with one linear combination under caller-chosen weights r_i and TWO pairings, instead of two pairings
 * per opening.  Jobs lie in flat arrays exactly as for plk_kzg_verify_batch, plus one weight byte per job;
 * a call holds n groups of m consecutive jobs each (m uniform over the call, as k is in
 * plk_kzg_verify_fold_batch): group g owns jobs [g m, (g + 1) m).  The weights are the caller's, as
 * everywhere in this library.
 *
 * CAVEAT.  An accepting aggregate is a statement about the WEIGHTED SUM of the group, not about each job:
 * a job with r_i = 0 is not checked at all, and wrong jobs whose weighted errors cancel are accepted.  That
 * the weights make this unlikely (independent, unpredictable to whoever produced the openings) is the
 * caller's business; with 17 possible weights no choice makes it negligible.
 *
 * Semantics (the specification: the reference's raw formulas applied blindly, as plk_kzg_verify_batch
 * applies them), group g:
 *   accL = accW = g1_identity();
 *   for i over the group's jobs in order:
 *       yG = g1_mul(&G, y_i); nyG = g1_neg(&yG); zW = g1_mul(&W_i, z_i);      (G = vk->g1)
 *       L = g1_add(&C_i, &nyG); L = g1_add(&L, &zW);
 *       t = g1_mul(&L, r_i);   accL = g1_add(&accL, &t);
 *       u = g1_mul(&W_i, r_i); accW = g1_add(&accW, &u);
 *   ok[g] = gtp_equal(pairing(&accL, &vk->g2_1), pairing(&accW, &vk->g2_s))     1 or 0
 * A group with an invalid byte (a G1 coordinate >= 101, a G1 flag > 1, z, y or r >= 17) gets ok[g] = 2; its
 * neighbours are unaffected.  m = 1 with r = 1 is plk_kzg_verify_batch's byte (g1_mul(L, 1) =
 * g1_add(identity, L) = L).
 *
 * Fast path: every C_i and W_i of the group and vk->g1 canonical group elements (the identity {0, 0, 1} or an
 * on-curve affine point with flag 0: the MSM's notion).  Then accL and accW are EXP of two sums of discrete
 * logs over the group's 9 bytes per job, and the group costs one streaming pass and two pairings.
 *   _dev form (asynchronous on `stream`): a group that is valid but not canonical -- and every valid group
 *   when vk->g1 is not canonical -- gets ok[g] = PLK_KZG_AGG_UNDECIDED (the `irregular` convention of
 *   plk_msm_g1_dev); its neighbours are unaffected.  Exactly n bytes of d_ok are written.  Pointers may have
 *   any alignment (the pass takes 16-byte loads in a group whose five arrays are 16-byte aligned at its first
 *   job, byte loads otherwise, with the same result); d_work is 4-byte aligned.
 *   Host form (synchronous): resolves those groups exactly -- the raw L_i, the library's exact raw fold over
 *   (L, r) and (W, r), the two pairings -- so it is exact for every valid input and never returns 3.
 * Geometry depends on (m, n) only.  plk_kzg_verify_agg_plan (host only, no device touched) reports it:
 *   out[0]  path: 0 one lane per group (the pairings in that lane), 1 one wave per group, 2 out[1] blocks per group
 *   out[1]  records per group in d_work (0 on path 0)
 *   out[2]  blocks of the first launch
 *   out[3]  launches: 1, or 2 -- the streaming pass, then one lane or wave per group finishing its records
 * d_work: plk_kzg_verify_agg_workspace(m, n) bytes (16 per record), 0 exactly where the plan says one launch,
 * and d_work may then be NULL.  Neither d_work nor d_ok needs initialisation: every word read was written by
 * the same call, no atomics are used, a workspace may be reused by the next call on the stream, and calls on
 * different streams with distinct workspaces may run concurrently.  Results are bit-identical from run to run.
 * Errors (before any device query): a NULL pointer (d_work only where the workspace is not 0), m == 0, n == 0
 * or an invalid byte in vk are PLK_ERR_ARG; m n > 2^30 is PLK_ERR_RANGE; the plan returns the same codes for
 * (m, n) and the workspace function 0.  No GPU is PLK_ERR_NODEV -- there is no CPU fallback.  The device
 * rules are those of plk_kzg_verify_batch(_dev). */
#define PLK_KZG_AGG_UNDECIDED 3
int    plk_kzg_verify_agg_plan(size_t m, size_t n, int64_t out[4]);          /* host only */
size_t plk_kzg_verify_agg_workspace(size_t m, size_t n);                     /* host only; 0: bad args or none needed */
int plk_kzg_verify_agg_batch(const plk_kzg_vk_t *vk, size_t m, const uint8_t *commits3, const uint8_t *zs,
                             const uint8_t *ys, const uint8_t *proofs3, const uint8_t *rs, size_t n, uint8_t *ok /* n */);
int plk_kzg_verify_agg_batch_dev(const plk_kzg_vk_t *vk /* HOST */, size_t m, const uint8_t *d_commits3,
                                 const uint8_t *d_zs, const uint8_t *d_ys, const uint8_t *d_proofs3,
                                 const uint8_t *d_rs, size_t n, uint8_t *d_ok, void *d_work, void *stream);

/* ---- KZG per-point openings: one polynomial at a point set, a proof each -----------------------
 * The producer the aggregate verification consumes: polynomial i is opened at every point of its set S_i
 * with a SEPARATE proof per point (vector commitments, data-availability samples: each position goes to a
 * different verifier, so the multi-point scheme's one proof for the whole set is no use).  A set is a
 * uint32_t mask as in the multi-point calls -- bit a set means a in S_i, bits 0 .. 16 only, at least one
 * bit -- but here ALL 17 bits is allowed: no divisor is ever formed.
 *
 * Job order: polynomials in call order, within a polynomial its points ascending;
 *   job e = sum_{i' < i} popcount(S_i') + rank of a in S_i,        J = sum_i popcount(S_i) jobs in all.
 * Every output array is flat in that order, so (d_zs, d_ys, d_proofs3) -- with the commitment repeated per
 * job, or a caller-made gather of it -- are the arguments of plk_kzg_verify_batch_dev and
 * plk_kzg_verify_agg_batch_dev as they are, without a host round trip.
 *
 * Semantics (the specification): job e = (i, a) returns exactly (ys[b], proofs3[3 b ..]) of
 * plk_kzg_open_batch on the expanded list whose entry b is (polys[i], lens[i], z = a); zs[e] = a where a zs
 * array is given.  This holds for every coefficient byte and any SRS in the host form.  Quotients are not
 * returned (plk_kzg_open_batch_dev stores them); len == 1 gives the identity proof and y = the coefficient.
 *   Host form (synchronous): a polynomial with a byte >= 17, and every polynomial when plk_srs_irregular, is
 *   recomputed by plk_kzg_open_batch itself on its expanded jobs.
 *   _dev form (asynchronous on `stream`): d_status[e] = 0 and the exact bytes on the fast path (canonical
 *   coefficients, regular SRS).  Every job of a polynomial with a byte >= 17 gets d_status = 1 and the proof
 *   bytes FF FF FF, which the verify calls answer with 2, never with an accept; its d_ys are unspecified.
 *   With an irregular SRS every job is flagged the same way while d_ys stay exact.  Neighbours are
 *   unaffected.  Exactly J bytes of d_zs, d_ys and d_status and 3 J bytes of d_proofs3 are written.
 * A polynomial's bytes and the SRS logs are read once for all its points (plus once more for the aggregates
 * when it exceeds 4096 coefficients); PLK_KZG_POINTS_LAUNCH_POLYS polynomials travel per launch, larger
 * batches run as consecutive launches on the stream.
 * d_work: plk_kzg_points_workspace bytes -- 4 x (points + non-zero points of the set) x chunks of 4096 for a
 * polynomial of more than one chunk, rounded up to 256 in all; 0 when every polynomial fits one chunk, and
 * d_work may then be NULL.  It needs no initialisation: every word read was written by the same call, no
 * atomics are used, it may be reused by the next call on the stream, and calls on different streams with
 * distinct workspaces may run concurrently.  Results are bit-identical from run to run.  Pointers may have
 * any alignment (d_work 4 bytes); 16-byte aligned polynomials take vector loads, with the same result.
 * d_polys, lens and sets are HOST arrays, d_polys holds device pointers (as plk_kzg_open_batch_dev).
 * Errors (all but the device check before any device query): a NULL handle or array (zs may be NULL), n <= 0,
 * lens[i] == 0, or a mask that is 0 or has a bit above 16 are PLK_ERR_ARG; max(lens[i] - 1, 1) > plk_srs_len
 * is PLK_ERR_RANGE with the reference's "degree exceeds SRS size" text; J > 2^30 is PLK_ERR_RANGE; a call
 * from another device is PLK_ERR_ARG.  No GPU is PLK_ERR_NODEV -- there is no CPU fallback. */
#define PLK_KZG_POINTS_LAUNCH_POLYS 64   /* polynomials one launch carries */
size_t plk_kzg_points_count(const uint32_t *sets, int n);                         /* J; host only; 0: bad args */
size_t plk_kzg_points_workspace(const size_t *lens, const uint32_t *sets, int n); /* host only; 0: bad args or none needed */
int plk_kzg_open_points_batch(const plk_srs_t *s, const uint8_t *const *polys, const size_t *lens,
                              const uint32_t *sets, int n,
                              uint8_t *zs /* J or NULL */, uint8_t *ys /* J */, uint8_t *proofs3 /* 3 J */);
int plk_kzg_open_points_batch_dev(const plk_srs_t *s, const uint8_t *const *d_polys, const size_t *lens,
                                  const uint32_t *sets, int n,
                                  uint8_t *d_zs /* J or NULL */, uint8_t *d_ys /* J */, uint8_t *d_proofs3 /* 3 J */,
                                  uint8_t *d_status /* J */, void *d_work, void *stream);

/* ---- KZG flat batches: many short polynomials committed and opened in one launch ------------------
 * The producer at the scale of the flat verify calls: vector commitments of a few dozen coefficients, the
 * per-row commitments of a table, the openings of very many small provers.  One call takes npoly polynomials
 * of at most PLK_KZG_FLAT_MAX coefficients each as consecutive segments of ONE flat coefficient array, with
 * device-side descriptors, and is ONE kernel launch whatever npoly is.  Every output is a flat device array
 * -- three bytes per G1, one byte per y and per status -- so (d_commits3, d_zs, d_ys, d_proofs3) of one
 * plk_kzg_open_flat_dev call are the arguments of plk_kzg_verify_batch_dev and plk_kzg_verify_agg_batch_dev as
 * they stand, without a host round trip.  (plk_kzg_commit_batch_dev / plk_kzg_open_batch_dev stay the calls for
 * a few LONG polynomials; plk_msm_g1_segments serves arbitrary points, not the SRS prefix every polynomial
 * needs here.)
 *
 * Segments, as in plk_msm_g1_segments.  Polynomial g is the bytes [o_g, o_{g+1}) of the flat array.
 *   uniform (d_offsets == NULL): o_g = g m and total == m npoly.
 *   ragged  (d_offsets != NULL): o_g = d_offsets[g], npoly + 1 words.  m is the largest length the caller
 *           allows: the launch geometry must not depend on device data, so the library needs this bound --
 *           and the list pays for it: bounded by m = 1024, a list whose polynomials are mostly short leaves
 *           most lanes of its waves idle.  Bucket by length (m <= 32, <= 1024, <= 4096) for speed.
 *   Every offset is read as min(o, total): no offset value whatever makes a kernel read outside [0, total)
 *   of the coefficients or outside the npoly + 1 offset words.
 * Semantics (the specification).  With status 0, polynomial g returns exactly the bytes plk_kzg_commit_batch
 * or plk_kzg_open_batch return for the expanded list whose entry g is (coeffs + o_g, o_{g+1} - o_g, zs[g]);
 * a length of 1 gives the identity proof and y = the coefficient.
 *   _dev forms (asynchronous on `stream`; d_zs is a DEVICE array):
 *     commitments are exact for ANY coefficient byte over a regular SRS (g1_mul takes the raw byte);
 *     a polynomial holding a byte >= 17 gets status PLK_KZG_FLAT_IRREGULAR from the opening call, proof bytes
 *       FF FF FF and an unspecified y; its commitment, where asked for, is still exact;
 *     with an irregular SRS every polynomial gets PLK_KZG_FLAT_IRREGULAR and FF FF FF in both G1 outputs,
 *       while the ys stay exact;
 *     PLK_KZG_FLAT_BAD, FF FF FF in every G1 output and y = FF: a ragged polynomial that is empty, has
 *       o_{g+1} < o_g, has an offset above total or is longer than m; and a polynomial whose device z byte is
 *       >= 17 (the host cannot see that byte).
 *     The verify calls answer FF FF FF with 2, never with an accept.  A flagged polynomial's neighbours are
 *     unaffected.  Exactly npoly bytes of d_ys and d_status and 3 npoly bytes of each G1 output are written.
 *   Host forms (synchronous): offsets and zs are validated on the host (each of the bad cases above is
 *     PLK_ERR_ARG before any device query) and flagged polynomials are recomputed through plk_kzg_open_batch /
 *     plk_kzg_commit_batch: the calls are exact for every byte and any SRS and need no status.
 * Geometry depends on (m, npoly) only.  plk_kzg_flat_plan (host only, no device touched) reports it:
 *   out[0]  path: 0 lane (m <= 32: one lane per polynomial), 1 wave (m <= 1024: one wave per polynomial,
 *           sixteen coefficients per lane), 2 block (m <= 4096: one block per polynomial)
 *   out[1]  polynomials per block: 256, 4 or 1
 *   out[2]  blocks (capped at 2048: a block loops over the polynomials with the stride of the grid)
 *   out[3]  launches: 1
 * No workspace, no memset, no atomics, no records: every word read was written by the caller, results are
 * bit-identical from run to run, and calls on different streams may run concurrently.  Pointers may have any
 * alignment (offsets 4 bytes); aligned coefficients take 16-byte loads, with the same result.
 * Errors.  The shape is checked first, then the pointers, then the SRS bound, then the device; all but the
 * last before any device query.  PLK_ERR_ARG: npoly == 0, total == 0 or m == 0; uniform with m npoly != total;
 * a NULL handle or a NULL required pointer; offsets off a 4-byte boundary; a call from another device.
 * PLK_ERR_RANGE: m > PLK_KZG_FLAT_MAX; total >= 2^32; npoly > 2^30; commitments asked for with m > plk_srs_len
 * or proofs with max(m - 1, 1) > plk_srs_len (the reference's "degree exceeds SRS size", on m as given).
 * plk_kzg_flat_plan returns the same codes for its arguments (its total is m npoly in uniform form).  No GPU
 * is PLK_ERR_NODEV -- there is no CPU fallback. */
#define PLK_KZG_FLAT_MAX 4096        /* coefficients per polynomial (one chunk of the opening kernels) */
#define PLK_KZG_FLAT_IRREGULAR 1     /* status: a coefficient byte >= 17 (openings), or an SRS without log form */
#define PLK_KZG_FLAT_BAD       2     /* status (_dev): a broken ragged segment, or a device z byte >= 17 */
int plk_kzg_flat_plan(size_t m, size_t npoly, int ragged, int64_t out[4]);            /* host only */
int plk_kzg_commit_flat_dev(const plk_srs_t *s, const uint8_t *d_coeffs, size_t total,
                            const uint32_t *d_offsets /* DEVICE, npoly + 1 words, or NULL */, size_t m, size_t npoly,
                            uint8_t *d_commits3 /* 3 npoly */, uint8_t *d_status /* npoly */, void *stream);
int plk_kzg_open_flat_dev(const plk_srs_t *s, const uint8_t *d_coeffs, size_t total,
                          const uint32_t *d_offsets, size_t m, size_t npoly, const uint8_t *d_zs /* DEVICE, npoly */,
                          uint8_t *d_ys /* npoly */, uint8_t *d_proofs3 /* 3 npoly */,
                          uint8_t *d_commits3 /* 3 npoly, or NULL */, uint8_t *d_status /* npoly */, void *stream);
int plk_kzg_commit_flat(const plk_srs_t *s, const uint8_t *coeffs, size_t total, const uint32_t *offsets /* host, or NULL */,
                        size_t m, size_t npoly, uint8_t *commits3);
int plk_kzg_open_flat(const plk_srs_t *s, const uint8_t *coeffs, size_t total, const uint32_t *offsets,
                      size_t m, size_t npoly, const uint8_t *zs, uint8_t *ys, uint8_t *proofs3,
                      uint8_t *commits3 /* or NULL */);

/* ---- KZG flat folded openings: many groups of short polynomials, one proof a group, one launch ----
 * The producer at the scale of plk_kzg_verify_fold_batch_dev: ngroups groups of k polynomials each, group g
 * opened at its one point zs[g] with ONE proof under per-polynomial weights -- PLONK's round 5 (nine
 * polynomials at z under powers of v) for very many small provers.  The polynomials are the segments of ONE
 * flat coefficient array exactly as in "KZG flat batches" above; weights and points are DEVICE arrays; the call
 * is ONE kernel launch whatever ngroups is.  (plk_kzg_open_fold_batch_dev stays the call for a few groups of
 * LONG polynomials.)
 *
 * Layout.  Polynomial e is the bytes [o_e, o_{e+1}) of the flat array: uniform (d_offsets == NULL) o_e = e m
 * and total == m k ngroups; ragged k ngroups + 1 device offset words, m the largest length the caller allows,
 * every offset read as min(o, total).  Group g owns polynomials [k g, k (g + 1)), weights [k g, k (g + 1)),
 * ys [k g, k (g + 1)) and the point zs[g]; k is uniform over a call, 1 <= k <= PLK_KZG_FOLD_MAX -- the
 * convention of plk_kzg_verify_fold_batch.  (d_commits3, d_weights, d_ys, d_zs, d_proofs3) of one call are the
 * arguments of plk_kzg_verify_fold_batch_dev(vk, k, .., n = ngroups, ..) with nothing moved.
 * Semantics (the specification).  With status 0, group g returns exactly the bytes of the library's own host
 * calls on the expanded group: ys[k g + i] and proofs3[3 g ..] those of plk_kzg_open_fold_batch for (the k
 * polynomials, their weights, zs[g]) -- polynomials of different lengths inside a group (L is the longest),
 * all weights zero, an F that cancels to a shorter degree or to zero, L = 1 (the identity proof) and z = 0
 * included -- and commits3[3 (k g + i) ..] that of plk_kzg_commit_batch.
 *   _dev form (asynchronous on `stream`), one status byte per GROUP; a group's neighbours are never affected:
 *     PLK_KZG_FLAT_BAD: a ragged polynomial of the group that is empty, falls, has an offset above total or is
 *       longer than m; a device z byte >= 17; a device weight byte >= 17 in the group.  The proof is
 *       FF FF FF, every y of the group FF and every commitment of the group FF FF FF.
 *     PLK_KZG_FLAT_IRREGULAR: a coefficient byte >= 17 anywhere in the group.  The proof is FF FF FF and the
 *       group's ys are unspecified; its commitments are still exact (g1_mul takes the raw byte).
 *     With an SRS that has no log form every group gets PLK_KZG_FLAT_IRREGULAR and FF FF FF in every G1
 *       output; the ys stay exact wherever the coefficients are canonical.
 *     Exactly k ngroups bytes of d_ys, 3 ngroups of d_proofs3, ngroups of d_status and, when given,
 *     3 k ngroups of d_commits3 are written.
 *   Host form (synchronous): offsets, weights and zs are validated on the host (each of the BAD cases above is
 *     PLK_ERR_ARG before any device query) and flagged groups are recomputed through plk_kzg_open_fold_batch /
 *     plk_kzg_commit_batch: the call is exact for every byte and any SRS and needs no status.
 * Geometry depends on (m, k, ngroups, ragged) only -- in fact on (m, ngroups).  plk_kzg_fold_flat_plan (host
 * only, no device touched) reports it, by the rule of plk_kzg_flat_plan:
 *   out[0]  path: 0 lane (m <= 32: one lane per group), 1 wave (m <= 1024: one wave per group, sixteen
 *           coefficients per lane), 2 block (m <= 4096: one block per group)
 *   out[1]  groups per block: 256, 4 or 1
 *   out[2]  blocks (capped at 2048: a block loops over the groups with the stride of the grid)
 *   out[3]  launches: 1
 * No workspace, no memset, no atomics, no records: every word read was written by the caller, results are
 * bit-identical from run to run, and calls on different streams may run concurrently.  Pointers may have any
 * alignment (offsets 4 bytes).
 * Errors.  The shape is checked first, then the pointers, then the SRS bound, then the device; all but the
 * last before any device query.  PLK_ERR_ARG: m, k, ngroups or total equal to 0; k > PLK_KZG_FOLD_MAX; uniform
 * with m k ngroups != total; a NULL handle or a NULL required pointer; offsets off a 4-byte boundary; a call
 * from another device.  PLK_ERR_RANGE: m > PLK_KZG_FLAT_MAX; total >= 2^32; k ngroups > 2^30;
 * max(m - 1, 1) > plk_srs_len, or m > plk_srs_len when commitments are asked for (the reference's "degree
 * exceeds SRS size", on m as given).  plk_kzg_fold_flat_plan returns the same shape codes (its total is
 * m k ngroups in uniform form).  No GPU is PLK_ERR_NODEV -- there is no CPU fallback. */
int plk_kzg_fold_flat_plan(size_t m, size_t k, size_t ngroups, int ragged, int64_t out[4]);   /* host only */
int plk_kzg_open_fold_flat_dev(const plk_srs_t *s, const uint8_t *d_coeffs, size_t total,
                               const uint32_t *d_offsets /* DEVICE, k ngroups + 1 words, or NULL */,
                               size_t m, size_t k, size_t ngroups,
                               const uint8_t *d_weights /* DEVICE, k ngroups */, const uint8_t *d_zs /* DEVICE, ngroups */,
                               uint8_t *d_ys /* k ngroups */, uint8_t *d_proofs3 /* 3 ngroups */,
                               uint8_t *d_commits3 /* 3 k ngroups, or NULL */, uint8_t *d_status /* ngroups */,
                               void *stream);
int plk_kzg_open_fold_flat(const plk_srs_t *s, const uint8_t *coeffs, size_t total, const uint32_t *offsets,
                           size_t m, size_t k, size_t ngroups, const uint8_t *weights, const uint8_t *zs,
                           uint8_t *ys, uint8_t *proofs3, uint8_t *commits3 /* or NULL */);

/* ---- KZG flat multi-point openings: many groups, each polynomial at its own point set, one launch ----
 * The producer at the scale of plk_kzg_verify_multi_batch_dev: ngroups groups of k polynomials each, polynomial
 * i of a group opened at every point of its own set S_i, the group answered by the two G1 elements W and W' of
 * "KZG multi-point openings" above -- PLONK's round 5 as it really is (eight polynomials at {z}, one at
 * {z, z omega}) for very many small provers.  The polynomials are the segments of ONE flat coefficient array
 * exactly as in "KZG flat folded openings"; sets, weights and challenges are DEVICE arrays; the call is ONE
 * kernel launch whatever ngroups, k and the sets are.  (plk_kzg_open_multi_batch_dev stays the call for a few
 * groups of LONG polynomials, and the one that returns h.)
 *
 * Layout.  Polynomial e is the bytes [o_e, o_{e+1}) of the flat array: uniform (d_offsets == NULL) o_e = e m
 * and total == m k ngroups; ragged k ngroups + 1 device offset words, m the largest length the caller allows,
 * every offset read as min(o, total).  Group g owns polynomials, masks, weights and 17-byte ys rows
 * [k g, k (g + 1)), the challenge us[g] and the six bytes proofs6[6 g ..] = W then W'; k is uniform over a
 * call, 1 <= k <= PLK_KZG_MULTI_MAX.  Masks follow the rules of the multi-point calls: non-zero, bits 0 .. 16
 * only, not all 17.  (d_commits3, d_sets, d_weights, d_ys, d_us, d_proofs6) of one call are the arguments of
 * plk_kzg_verify_multi_batch_dev(vk, k, .., n = ngroups, ..) with nothing moved; d_sets is therefore 4-byte
 * aligned.  h is not returned: there is no d_hs in the flat form.
 * Semantics (the specification).  With status 0, group g returns exactly the bytes of the library's own host
 * calls on the expanded group: ys[17 (k g + i) ..] and proofs6[6 g ..] those of plk_kzg_open_multi_batch for
 * (the k polynomials, their masks, their weights, us[g]) -- all 17 bytes of a row are written, 0xFF off the
 * set; len_i <= |S_i|, all weights zero, an h that cancels to zero or to a shorter degree, u inside T, outside
 * T and u = 0, the point 0 in a set, a set of 16 points, polynomials of different lengths in a group and m = 1
 * included -- and commits3[3 (k g + i) ..] that of plk_kzg_commit_batch.
 *   _dev form (asynchronous on `stream`), one status byte per GROUP; a group's neighbours are never affected:
 *     PLK_KZG_FLAT_BAD: a ragged polynomial of the group that is empty, falls, has an offset above total or is
 *       longer than m; an invalid mask; a device weight byte >= 17; a device u byte >= 17.  Both proofs are
 *       FF FF FF, every one of the group's 17 k ys bytes FF and every commitment of the group FF FF FF.
 *     PLK_KZG_FLAT_IRREGULAR: a coefficient byte >= 17 anywhere in the group.  Both proofs are FF FF FF and the
 *       group's ys are unspecified; its commitments are still exact (g1_mul takes the raw byte).
 *     With an SRS that has no log form every group gets PLK_KZG_FLAT_IRREGULAR and FF FF FF in every G1
 *       output; the ys stay exact wherever the coefficients are canonical.
 *     Exactly 17 k ngroups bytes of d_ys, 6 ngroups of d_proofs6, ngroups of d_status and, when given,
 *     3 k ngroups of d_commits3 are written.  No offset, mask, weight or u value makes a kernel read outside
 *     the arrays as sized here.
 *   Host form (synchronous): offsets, masks, weights and us are validated on the host (each of the BAD cases
 *     above is PLK_ERR_ARG before any device query) and flagged groups are recomputed through
 *     plk_kzg_open_multi_batch / plk_kzg_commit_batch: the call is exact for every byte and any SRS and needs
 *     no status.
 * Geometry depends on (m, k, ngroups, ragged) only -- in fact on (m, ngroups).  plk_kzg_multi_flat_plan (host
 * only, no device touched) reports it, by the rule of plk_kzg_flat_plan:
 *   out[0]  path: 0 lane (m <= 32: one lane per group), 1 wave (m <= 1024: one wave per group, sixteen
 *           coefficients per lane), 2 block (m <= 4096: one block per group)
 *   out[1]  groups per block: 256, 4 or 1
 *   out[2]  blocks (capped at 2048: a block loops over the groups with the stride of the grid)
 *   out[3]  launches: 1
 * No workspace, no memset, no atomics, no records: every word read was written by the caller, results are
 * bit-identical from run to run, and calls on different streams may run concurrently.  Coefficients and outputs
 * may have any alignment (offsets and sets 4 bytes).
 * Errors.  The shape is checked first, then the pointers, then the SRS bound, then the device; all but the
 * last before any device query.  PLK_ERR_ARG: m, k, ngroups or total equal to 0; k > PLK_KZG_MULTI_MAX; uniform
 * with m k ngroups != total; a NULL handle or a NULL required pointer; offsets or sets off a 4-byte boundary; a
 * call from another device.  PLK_ERR_RANGE: m > PLK_KZG_FLAT_MAX; total >= 2^32; k ngroups > 2^30;
 * max(m - 1, 1) > plk_srs_len, or m > plk_srs_len when commitments are asked for (Lh <= max(m - 1, 1), and W'
 * commits at most max(m - 1, 1) quotient bytes).  plk_kzg_multi_flat_plan returns the same shape codes (its
 * total is m k ngroups in uniform form).  No GPU is PLK_ERR_NODEV -- there is no CPU fallback. */
int plk_kzg_multi_flat_plan(size_t m, size_t k, size_t ngroups, int ragged, int64_t out[4]);   /* host only */
int plk_kzg_open_multi_flat_dev(const plk_srs_t *s, const uint8_t *d_coeffs, size_t total,
                                const uint32_t *d_offsets /* DEVICE, k ngroups + 1 words, or NULL */,
                                size_t m, size_t k, size_t ngroups,
                                const uint32_t *d_sets /* DEVICE, k ngroups masks */,
                                const uint8_t *d_weights /* DEVICE, k ngroups */,
                                const uint8_t *d_us /* DEVICE, ngroups */,
                                uint8_t *d_ys /* 17 k ngroups */, uint8_t *d_proofs6 /* 6 ngroups: W, W' */,
                                uint8_t *d_commits3 /* 3 k ngroups, or NULL */, uint8_t *d_status /* ngroups */,
                                void *stream);
int plk_kzg_open_multi_flat(const plk_srs_t *s, const uint8_t *coeffs, size_t total, const uint32_t *offsets,
                            size_t m, size_t k, size_t ngroups, const uint32_t *sets, const uint8_t *weights,
                            const uint8_t *us, uint8_t *ys, uint8_t *proofs6, uint8_t *commits3 /* or NULL */);

/* ---- device-resident prover (replaces plonk_new / plonk_prove / plonk_free,
 * src/plonk.h:53-139, 223-656, 120-139) ---------------------------------------------------
 * plk_prover_create uploads the SRS and Z_H once (the PLONK struct of plonk_new); the
 * circuit tables h, k1_h, k2_h, h_pows_inv are optional (needed only by plk_prover_prove).
 * h_pows_inv is the inverse Vandermonde matrix row-major, [r * n + c] = matrix_get(r, c).
 * A prover owns its stream and work buffers: one call at a time per plk_prover_t (distinct
 * provers may run from different threads).
 * Largest n: with a binomial Z_H (x^n - 1) a proof needs n <= 3,932,158.  Round 3's products run as
 * one exact transform each, over F29 or, past its range, BabyBear (p = 15 2^27 + 1), which holds a
 * product of bytes < 17 exactly while 256 min(la, lb) < p; t_2 = (A2 B2)(C2 z) has a shorter operand
 * of 2n + 3 coefficients, and (2n + 3) 256 < p gives the limit.  plk_prover_create accepts a larger
 * n; plk_prover_prove / plk_prover_rounds_dev then return PLK_ERR_RANGE ("outside the exact range")
 * before that batch's transforms are launched, and the prover can still be destroyed. */
typedef struct plk_prover plk_prover_t;
typedef struct {
  size_t n;                                  /* gates = |H| */
  const uint8_t *h, *k1_h, *k2_h;            /* n each (HF values), or NULL */
  const uint8_t *h_pows_inv;                 /* n * n, or NULL */
  const uint8_t *z_h;                        /* Z_H(x) coefficients (plonk.z_h_x) */
  size_t z_h_len;
  const uint8_t *srs_g1;                     /* srs.g1s, 3 bytes per G1 */
  size_t srs_len;
} plk_plonk_desc_t;
/* CONSTRAINTS + ASSIGNMENTS (src/constraints.h:11-60); copies are (type, index) byte pairs,
 * type 0 = COPYOF_A, 1 = COPYOF_B, 2 = COPYOF_C, index 1-based (n <= 16 in GF(17)) */
typedef struct {
  const uint8_t *q_m, *q_l, *q_r, *q_o, *q_c;
  const uint8_t *copy_a, *copy_b, *copy_c;   /* 2n bytes each */
  const uint8_t *a, *b, *c;
} plk_circuit_t;
#define PLK_PROVE_STRICT 1                   /* enforce the zero-remainder asserts */
int plk_prover_create(const plk_plonk_desc_t *desc, plk_prover_t **out);
void plk_prover_destroy(plk_prover_t *p);
size_t plk_prover_device_bytes(const plk_prover_t *p);
/* plonk_prove: chal = {alpha, beta, gamma, z, v}; proof = the 34-byte PROOF struct.  Errors
 * where the reference exits or asserts (unsatisfied gate, bad copy, SRS too short, non-zero
 * remainder, t(x) too short to slice) return PLK_ERR_ARG / PLK_ERR_RANGE. */
int plk_prover_prove(plk_prover_t *p, const plk_circuit_t *circuit, const uint8_t chal[5],
                     const uint8_t rand9[9], uint8_t proof[34]);
/* rounds 1-5 of plonk_prove from device-resident interpolated polynomials (each zero padded
 * to n bytes): f_a f_b f_c q_o q_m q_l q_r q_c s_sigma_1 s_sigma_2 s_sigma_3 acc_x l_1_x.
 * Without PLK_PROVE_STRICT non-zero remainders are tolerated (synthetic inputs).
 * The 13 pointers may have any alignment, each on its own; exactly n bytes of each are read and
 * none is written, whatever lies beside them.  16-byte aligned inputs take the fused kernels (the
 * one-launch rounds 1-3 preparation; with n % 16 == 0 also round 5's numerators inside the
 * division launch and the chunk aggregates); q_c 4-byte aligned with n % 4 == 0 keeps t(x)'s
 * numerator fused with its division.  Any other placement runs the byte-wise forms: more
 * launches, the same 34 bytes. */
int plk_prover_rounds_dev(plk_prover_t *p, const uint8_t *const d_polys[13], const uint8_t chal[5],
                          const uint8_t rand9[9], int flags, uint8_t proof[34]);
/* Many whole proofs in one call (throughput proving of small circuits: many witnesses of one
 * circuit, many challenge or blinding draws).  Entry b of plk_prover_prove_batch is
 * plk_prover_prove(p, circuit b, chal b, rand b), circuit b being the 14 n bytes
 *   q_m q_l q_r q_o q_c (n each) | copy_a copy_b copy_c (2n each, (type, index) pairs) | a b c (n each);
 * entry b of plk_prover_rounds_batch is plk_prover_rounds_dev on the 13 polynomials of entry b (in its
 * order, each zero padded to n bytes, entries 13 n bytes apart) with `flags` (PLK_PROVE_STRICT only;
 * PLK_PROVE_PREPROCESSED is PLK_ERR_ARG).  An accepted entry gets the same 34 bytes and status 0; a
 * rejected one 34 zero bytes and the status word below: the exit the single call would take, in its
 * order.  One deliberate difference: a rounds_batch entry with a polynomial byte >= 17 takes the
 * exit INPUT (PLK_ERR_ARG); its neighbours are unaffected.  The return value covers the call only:
 * PLK_OK means every entry was processed, whatever the statuses.
 *   per-entry status word: 0 = proof written; else
 *     bits 0-7   the PLK_ERR_* code the single call would return,
 *     bits 8-15  the exit: 1 GATE, 2 COPY, 3 SRS, 4 ACC, 5 REM_T, 6 SLICE, 7 REM_W1, 8 REM_W2, 9 INPUT,
 *     bits 16-31 the gate index for GATE (the %u of "Constraint %u not satisfied.")
 * Fused path (plk_prover_batch_path = 1): n <= PLK_PROVE_BATCH_MAX_N, a regular SRS (the prover's log
 * form exists) and a canonical trimmed Z_H of length 2..n + 1: ONE kernel launch proves the whole
 * batch, one wave per proof.  Otherwise (path 0) the host forms run the composition itself, one
 * single call per entry, status and message from that call's return; the _dev forms (DEVICE arrays,
 * asynchronous on `stream`, the fused path only) return PLK_ERR_RANGE.  The host forms stage through
 * buffers owned by the prover, grown on demand and counted in plk_prover_device_bytes.
 * Errors (checked before any device query): NULL arrays, batch <= 0 (PLK_ERR_ARG), batch > 1 << 24
 * (PLK_ERR_RANGE), the circuit form on a prover created without tables, a call from another device
 * (PLK_ERR_ARG).  One call at a time per prover; attached helpers are ignored. */
#define PLK_PROVE_BATCH_MAX_N 16
/* the text plk_last_error() holds after the single call that takes this exit, NUL-terminated and
 * truncated to cap bytes; returns its full length (0 for status 0), -PLK_ERR_ARG for an unknown exit.
 * Host only, no device. */
int plk_prove_exit_message(uint32_t status, char *buf, size_t cap);
/* 1 fused kernel, 0 composition, -PLK_ERR_* (NULL prover; circuit != 0 without tables); host only */
int plk_prover_batch_path(const plk_prover_t *p, int circuit);
int plk_prover_prove_batch(plk_prover_t *p, const uint8_t *circuits /* batch x 14n */,
                           const uint8_t *chals /* 5 each */, const uint8_t *rands /* 9 each */, int batch,
                           uint8_t *proofs /* 34 each */, uint32_t *status);
int plk_prover_rounds_batch(plk_prover_t *p, const uint8_t *polys /* batch x 13 x n */, const uint8_t *chals,
                            const uint8_t *rands, int flags, int batch, uint8_t *proofs, uint32_t *status);
int plk_prover_prove_batch_dev(plk_prover_t *p, const uint8_t *d_circuits, const uint8_t *d_chals,
                               const uint8_t *d_rands, int batch, uint8_t *d_proofs, uint32_t *d_status,
                               void *stream);
int plk_prover_rounds_batch_dev(plk_prover_t *p, const uint8_t *d_polys, const uint8_t *d_chals,
                                const uint8_t *d_rands, int flags, int batch, uint8_t *d_proofs,
                                uint32_t *d_status, void *stream);

/* Preprocessed circuit (PLONK's preprocessed input; the reference re-derives it inside every
 * plonk_prove, src/plonk.h:386-503): the forward transforms round 3 needs of the fixed circuit
 * polynomials q_o q_m q_l q_r s_sigma_3 l_1_x (d_polys indices 3 4 5 6 10 12, device-resident,
 * zero padded to n) are computed once here.  plk_prover_rounds_dev with PLK_PROVE_PREPROCESSED
 * then uses them for the entries whose address equals the one given here; the bytes at those
 * addresses must not change while they are in use (call again after a change; d_polys = NULL
 * drops them).  Proof bytes are identical with and without.  The six pointers may have any
 * alignment; exactly n bytes of each are read here, and nothing of the caller's is written. */
#define PLK_PROVE_PREPROCESSED 2
int plk_prover_preprocess(plk_prover_t *p, const uint8_t *const d_polys[13]);
/* Measurement of one proof (bench.py's C5 roofline; no reference counterpart).
 * plk_prover_profile_dev = plk_prover_rounds_dev (same bytes) with hipEvents on the prover's stream
 * around its whole launch sequence and around each of round 3's two product batches -- every NTT
 * pass kernel of the proof; ms = {launch sequence, both batches, batch 1, batch 2} in milliseconds
 * (one prover, no helpers).
 * plk_prover_launches: the kernel launches (and other graph nodes: copies, memsets) of one such
 * call, counted by capturing it as a HIP graph that is never launched (nothing runs, no state
 * changes).
 * plk_prover_alg_bytes: rounds 1-5's algorithmic bytes in SURVEY 8(d) terms over the reference's own
 * ops (src/plonk.h:277-621): 17 poly_mul at la + lb + (la + lb - 1), 9 srs_eval_at_s at 4 B per point,
 * 3 poly_divide (operands read, quotient and remainder written), 9 poly_eval (one read each). */
int plk_prover_profile_dev(plk_prover_t *p, const uint8_t *const d_polys[13], const uint8_t chal[5],
                           const uint8_t rand9[9], int flags, uint8_t proof[34], double ms[4]);
int plk_prover_launches(plk_prover_t *p, const uint8_t *const d_polys[13], const uint8_t chal[5],
                        const uint8_t rand9[9], int flags, int *kernels, int *other_nodes);
uint64_t plk_prover_alg_bytes(const plk_prover_t *p);

/* Strong-scaled proof over several GPUs (round 3's independent poly_mul jobs spread
 * across GPUs as whole jobs).  Two of round 3's product chains depend only on the proof's inputs:
 *   PLK_CHAIN_T2: t_2 = (A2 B2)(C2 z_x)            (src/plonk.h:432-434, re-associated)
 *   PLK_CHAIN_T3: t_3 = (A3 B3)(C3 z_x(omega x))   (src/plonk.h:471-473)
 * A helper GPU computes them from the same inputs as the proving GPU with plk_prover_chains_dev;
 * their bytes travel to the proving GPU (e.g. an RCCL send / receive), whose
 * plk_prover_rounds_ext_dev skips those chains and reads the bytes instead.  The proof bytes are
 * identical to plk_prover_rounds_dev's.  Buffers: plk_prover_chain_bytes(p, chain) bytes each,
 * 16-byte aligned, device memory of the prover's GPU. */
#define PLK_CHAIN_T2 1
#define PLK_CHAIN_T3 2
size_t plk_prover_chain_bytes(const plk_prover_t *p, int chain);
/* Enqueue rounds 1-3's preparation and the chains in `which` on the prover's stream, products
 * into d_t2 / d_t3; the stream `done` (NULL: the null stream) waits for them.  Returns without
 * waiting. */
int plk_prover_chains_dev(plk_prover_t *p, const uint8_t *const d_polys[13], const uint8_t chal[5],
                          const uint8_t rand9[9], int which, uint8_t *d_t2, uint8_t *d_t3, void *done);
/* plk_prover_rounds_dev with the chains in `which` read from d_t2 / d_t3, after everything
 * enqueued on stream `ready` (NULL: the null stream) at the time of the call -- e.g. their
 * receive. */
int plk_prover_rounds_ext_dev(plk_prover_t *p, const uint8_t *const d_polys[13], const uint8_t chal[5],
                              const uint8_t rand9[9], int flags, int which, const uint8_t *d_t2,
                              const uint8_t *d_t3, void *ready, uint8_t proof[34]);

/* The same split driven from C in one process, over the plk_init_devices list (no RCCL, no
 * caller-side hand-off): plk_prover_attach_helpers(p, k) creates k helper provers on list entries
 * 1..k (k = 1: t_3 on ids[1]; k = 2: t_2 on ids[1] and t_3 on ids[2]; 0 detaches; call from p's
 * device).  Afterwards plk_prover_rounds_dev and plk_prover_prove run every proof split: p's
 * stream records an event after the work already enqueued on it (the inputs); each helper's stream
 * waits for it, copies the 7 polynomials its chains read (f_a f_b f_c s_sigma_1..3 acc_x) to its
 * own GPU when that is another device (hipMemcpyPeerAsync), runs the chains, copies their products
 * into receive buffers on p's GPU (hipMemcpyPeerAsync on the helper's stream) and records an event;
 * p's stream waits for those events only before its numerator.  Ids may repeat (the one-GPU
 * rehearsal: helpers on their own streams of the same device).  Same proof bytes.
 * plk_prover_rounds_multi_dev takes the inputs already resident on every device: d_polys holds
 * ndev = 1 + k sets of 13 pointers, set 0 on p's device, set h on helper h's (no input copies). */
int plk_prover_attach_helpers(plk_prover_t *p, int k);
int plk_prover_helpers(const plk_prover_t *p);   /* the k attached (0: none) */
int plk_prover_rounds_multi_dev(plk_prover_t *p, const uint8_t *const *d_polys, int ndev, const uint8_t chal[5],
                                const uint8_t rand9[9], int flags, uint8_t proof[34]);

#ifdef __cplusplus
}
#endif
#endif /* PLONKHIP_H */
