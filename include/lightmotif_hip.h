/*
 * lightmotif_hip.h -- C ABI of the MI355X (gfx950) scoring back-end.
 *
 * This is the drop-in boundary for ONE hot path of althonos/lightmotif:
 *
 *     pssm.score(&striped)  ->  StripedScores  ->  argmax / max / threshold
 *
 * The reference has no FFI; its boundary is the trait surface
 * `Score` / `Maximum` / `Threshold` (+ `Stripe`, `Encode`) of
 * lightmotif/src/pli/mod.rs:34-222, implemented per back-end marker and fanned
 * out by `enum Dispatch` (lightmotif/src/pli/dispatch.rs:33-41).  A new
 * `Dispatch::Hip` arm (dispatch.rs:90-106, 160-177) -- or an out-of-crate type
 * implementing the public traits -- forwards raw pointers and dimensions to
 * the functions below (INTEGRATION.md has the Rust shim).  Every entry point
 * names the reference function it stands in for.
 *
 * Conventions
 *  - plain C types only; no C++ exceptions cross the boundary;
 *  - every function returns an `lm_hip_status`; `lm_hip_last_error()` gives the
 *    thread-local message of the last failure.  The reference's trait methods
 *    return ()/Option and *panic* on misuse (avx2.rs:832-837, 354-358); the shim
 *    turns a non-zero status into `panic!`.  Degenerate inputs are NOT errors:
 *    L < M or an empty row range gives zero rows (pli/mod.rs:85-88), empty
 *    scores give found = 0 (pli/mod.rs:136-138);
 *  - a NULL handle or a NULL required pointer is LM_HIP_ERR_BAD_ARGS (checked before any device
 *    work: the context stays usable); `*_destroy(NULL)` and lm_hip_free(NULL) are no-ops.  Outputs
 *    that may be NULL when the caller does not want them: `best` / `value` next to `found`
 *    (argmax, max, the batch argmax), `values` next to `coords` (threshold batch), `out_rows` /
 *    `max_index`, `bad_index` (tests/test_abi_exports.py, tests/test_gpu_abi_misuse.py);
 *  - memory layout is the reference's: striped sequence
 *    (rows+wrap) x stride bytes, PSSM M x stride f32 (stride 8 for DNA, 24 for
 *    protein), scores rows x stride f32, all row-major, `stride` in ELEMENTS
 *    (DenseMatrix::stride, dense.rs:126-128);
 *  - `*_dptr` functions take DEVICE pointers and enqueue on the context's
 *    stream; results that come back to the host (argmax, threshold, counts)
 *    synchronise that stream before returning.  Host-pointer functions are
 *    fully synchronous (the GPU analogue of the `_mm_sfence` at avx2.rs:198);
 *  - pointers, strides and alignment of the `*_dptr` functions and of lm_hip_seq_adopt_dptr: a device pointer needs
 *    the alignment of its ELEMENT only (f32 matrices: 4 bytes; u8 matrices, ASCII and symbol bytes: none), and every
 *    stride >= cols is accepted, whatever cols is -- a torch view with a storage offset, one row shard of a wider
 *    buffer, a matrix whose rows are wider than their live columns.  `seq_stride`, `out_stride` and `stride` are
 *    independent of each other.  The results, and the cells written, are the same at every placement: the bytes
 *    between `cols` and the stride of a row are never read, and never written except by Stripe / configure_wrap, which
 *    say so below.  No placement is refused; what depends on it is the KERNEL, hence the speed (lm_hip_ctx_last_kernel
 *    and lm_hip_ctx_launch_tally tell which one ran; tests/test_gpu_foreign_geometry.py holds the library to this list):
 *      . Score<f32> (store and fused forms): the unrolled kernels (score_c32<M,MODE>, the prefilter scans) need
 *        cols == 32 (the plain store: also 16) and seq_stride == 32, a store also out_stride == cols.  Otherwise a store
 *        runs the LDS-tiled kernel (score_tiled) or goes cell by cell, a fused form goes cell by cell
 *        (score_generic<1>, <2>).  The output pointer needs no more than its 4 bytes.
 *      . d_seq % 4 != 0 (natural strides): no kernel with dword symbol loads.  Stores of M <= 36 run the byte-load
 *        member of the family, longer motifs (the long and very long families, slices) the tiled kernel; fused forms
 *        scan one symbol per lookup with byte loads (no pair scan, no 4-row symbol blocks, no multi-motif pass) and
 *        go cell by cell beyond M = 36; Score<u8> looks one symbol up at a time; lm_hip_scan_max_f32 walks
 *        materialised windows.
 *      . Score<u8>: as Score<f32>, and d_out % 4 != 0 goes cell by cell (score_generic_u8).
 *      . Maximum / Threshold (f32 and u8): stride == cols with a 16-byte aligned pointer is read as one flat array,
 *        16 bytes per lane; anything else cell by cell.
 *      . Encode: 16 bytes per lane when source and destination are both 16-byte aligned, else byte by byte.
 *      . Stripe: cols == 32, stride == 32 and d_data % 16 == 0 stores 16 bytes per lane; d_data % 4 == 0 with
 *        stride % 4 == 0 stores dwords; anything else bytes.  configure_wrap is byte-wise throughout.
 *  - all entry points are thread-safe; a context serialises its own calls.
 */
#ifndef LIGHTMOTIF_HIP_H
#define LIGHTMOTIF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when an entry point is removed or changes its meaning.  Rounds 2-6 only ADDED entry points (the one removal, of
 * lm_hip_ctx_set_xcd_remap in round 5, was taken back: it is a no-op now), so a binding built against an earlier header
 * still loads and links. */
#define LM_HIP_ABI_VERSION 1

typedef enum lm_hip_status {
    LM_HIP_OK = 0,
    LM_HIP_ERR_BAD_ARGS = 1,    /* null pointer, stride < cols, rows out of range ... */
    LM_HIP_ERR_WRAP = 2,        /* "not enough wrapping rows for motif of length M" (avx2.rs:832-837) */
    LM_HIP_ERR_HIP = 3,         /* a HIP runtime call failed */
    LM_HIP_ERR_OOM = 4,         /* host or device allocation failed */
    LM_HIP_ERR_NO_DEVICE = 5,   /* no gfx950 device: maps to UnsupportedBackend (err.rs:34) */
    LM_HIP_ERR_INVALID_SYMBOL = 6, /* Encode: InvalidSymbol (err.rs:10) */
    LM_HIP_ERR_CAPACITY = 7,    /* caller-provided buffer too small (output list, adopted matrix) */
    LM_HIP_ERR_COMM = 8         /* RCCL missing, or a collective / communicator call failed */
} lm_hip_status;

/* (row, col) of a cell of a striped matrix -- dense.rs:28-39 MatrixCoordinates. */
typedef struct lm_hip_coords {
    size_t row;
    size_t col;
} lm_hip_coords;

/* One above-threshold position of the fused scan (scan.rs:52-75 `Hit`). */
typedef struct lm_hip_hit {
    size_t position; /* col * rows + row, scores.rs:155-157 */
    float score;
} lm_hip_hit;

/* One hit of a scan over a sequence set: the record and the position INSIDE that record (main.rs:527-531 writes
 * exactly this pair per line of the CLI's table). */
typedef struct lm_hip_set_hit {
    size_t record;
    size_t position;
    float score;
} lm_hip_set_hit;

/* The best window of one motif in one record of a sequence set (lm_hip_scan_best_seqset): 16 bytes. */
typedef struct lm_hip_set_best {
    uint64_t position; /* inside the record; 0 when found == 0 */
    float score;       /* NaN when found == 0 */
    int32_t found;
} lm_hip_set_best;

typedef struct lm_hip_ctx lm_hip_ctx;       /* device + stream + scratch */
typedef struct lm_hip_pssm lm_hip_pssm;     /* ScoringMatrix data resident on the device */
typedef struct lm_hip_seq lm_hip_seq;       /* StripedSequence resident on the device */
typedef struct lm_hip_seqset lm_hip_seqset; /* many records resident as one StripedSequence + their offsets */
typedef struct lm_hip_scores lm_hip_scores; /* StripedScores<f32> resident on the device */
typedef struct lm_hip_comm lm_hip_comm;     /* RCCL communicator of a row-sharded job */
typedef struct lm_hip_dists lm_hip_dists;   /* ScoreDistribution of n matrices resident on the device */

/* ---- library ------------------------------------------------------------ */

int lm_hip_abi_version(void);
const char *lm_hip_last_error(void);
/* Pipeline::avx2()/neon() -> Result<_, UnsupportedBackend> (pli/mod.rs:401-407):
 * number of usable devices; 0 devices is reported through *count, not an error. */
int lm_hip_device_count(int *count);
/* HIP ordinal of the index-th usable (gfx950) device, 0 <= index < lm_hip_device_count: the
 * value lm_hip_ctx_create and $LM_HIP_DEVICE take.  On a node with other GPUs in between,
 * iterate over this instead of range(count).  LM_HIP_ERR_NO_DEVICE past the end. */
int lm_hip_device_ordinal(int index, int *ordinal);
/* Frees buffers this library returned to the caller (threshold / hit lists). */
void lm_hip_free(void *p);
/* The pool behind large result arrays (threshold / hit lists): page-locked 2 MB-aligned blocks re-used between calls.
 * Bytes it holds idle, bytes handed out and not yet freed, and the idle budget ($LM_HIP_RESULT_POOL_MB, default 256;
 * blocks in use may reach four times that, results beyond come from plain malloc).  For hosts that watch their
 * locked memory; a pointer may be NULL (not all three). */
int lm_hip_result_pool_info(size_t *pinned_idle, size_t *pinned_in_use, size_t *budget);

/* Diagnostic: the shader clock (MHz) the device sustains over the next `window_us` microseconds, measured by one
 * mostly-sleeping wavefront on a stream of its own (s_memtime ticks per s_memrealtime tick) -- call it from
 * a second host thread while the kernels of interest run to learn the clock THEY get (the part clocks to its power
 * budget; a roofline priced at the 2.4 GHz of the data sheet is not what an LDS- or VALU-bound kernel can reach).
 * The probe's stream and record are made once per device and kept.  (Two marks enqueued IN the measured stream were tried
 * and dropped: the counter is per XCD and not comparable between the places two one-workgroup kernels land.)
 * No reference counterpart; bench.py reports it next to every LDS fraction. */
int lm_hip_device_clock_mhz(int device, unsigned window_us, double *mhz);

/* DenseMatrix::stride (dense.rs:126-128) for x86-64 hosts: elements per row. */
size_t lm_hip_stride(size_t cols, size_t elem_size);

/* ---- context ------------------------------------------------------------ */

/* `Pipeline::dispatch()` is re-created per call in the reference
 * (pwm/mod.rs:646, scores.rs:182); the GPU state it would need lives here. */
/* `device` is a HIP ordinal (what hipSetDevice / torch.device("cuda", i) / LOCAL_RANK use);
 * LM_HIP_ERR_NO_DEVICE if it is not a gfx950 device (lm_hip_device_ordinal lists those). */
int lm_hip_ctx_create(int device, lm_hip_ctx **out);
/* Borrow an existing hipStream_t (e.g. PyTorch's current stream) instead of
 * creating one.  The stream must outlive the context. */
int lm_hip_ctx_create_on_stream(int device, void *hip_stream, lm_hip_ctx **out);
int lm_hip_ctx_destroy(lm_hip_ctx *ctx);
int lm_hip_ctx_sync(lm_hip_ctx *ctx);
/* hipStream_t the context enqueues on (for hipEvent timing by the caller). */
int lm_hip_ctx_stream(lm_hip_ctx *ctx, void **hip_stream);
/* Tuning knob: output rows each wavefront half sweeps in the C=32 score
 * kernels (0 = library default). */
int lm_hip_ctx_set_rows_per_stream(lm_hip_ctx *ctx, size_t rows);
/* Tuning knob of the fused score+threshold scans (lm_hip_score_threshold_f32_dptr,
 * lm_hip_scan_f32, lm_hip_scan_threshold_batch): 1 (default) = candidates are found
 * with a packed 16-bit over-estimating discretisation of the PSSM (the GPU form of the
 * reference Scanner's DiscreteMatrix prefilter, scan.rs:169-198) and re-scored exactly;
 * 0 = every position is scored in f32.  The hit lists are identical either way. */
int lm_hip_ctx_set_prefilter(lm_hip_ctx *ctx, int enabled);
/* lm_hip_score_rows_into / lm_hip_score_into on handles: 1 (default) = for matrices of at least
 * 8 Mi cells the store kernel also tracks the maximum, and a following lm_hip_argmax on the
 * same lm_hip_scores (the reference's score_into + argmax flow, lightmotif-bench dna.rs:
 * 104-107) is a 16-byte read instead of a second pass over the matrix (1.65 -> 1.03 ms per
 * Gbp for the pair; the two tiny reduction launches add ~2 % to a score_into that is never
 * followed by argmax); 0 = plain store.  The cached result is invalidated by the library's
 * own writes to the handle -- not by external writes through the device pointer of
 * lm_hip_scores_info. */
int lm_hip_ctx_set_track_argmax(lm_hip_ctx *ctx, int enabled);
/* Selects an alternative path inside the library for this context.  Every option leaves the RESULTS unchanged (the
 * test-suite runs both sides of each against the oracle); they exist for A/B measurements and to exercise paths that
 * are otherwise taken only for some shapes.  Names: "track_argmax", "prefilter" (= the setters above),
 * "pair_prefilter", "pair_prefilter_protein", "speculate_order", "suffix_argmax", "suffix_occurrences", "multi_motif",
 * "skip_unreachable", "quad_loads", "xlong_store", "host_fold", "chunked_fused", "chunk_rows", "tiled", "sort_hits",
 * "short_order", "time_scan", "drop_last", "list_scan_max" (0 = Scanner::max always walks windows of materialised u8 scores),
 * "block_prefilter" (0 = the protein one-symbol scans load a byte per lane and row
 * instead of 4-row blocks), "poll_done" (1 = a single fused threshold call polls the word the ranking kernel raises in pinned
 * memory instead of waiting for its stream: 3-4 us less per call, unless the caller synchronises the device right behind it),
 * "count_tile_rows" (rows per block of the table behind lm_hip_seq_count_symbols / lm_hip_seqset_count_symbols, 1 ... 65536;
 * 0 = the default of 1024: a small value makes a small input span many blocks of the table and of its scan),
 * "site_chunk" (most sites per chunk of lm_hip_seqset_windows / lm_hip_seqset_count_sites, 0 = the default: a small value
 * makes a small list cross chunk boundaries),
 * "variant_chunk" (most variants per chunk of lm_hip_seqset_variant_effects / lm_hip_seqset_variant_hits, 0 = the default of
 * 2^20: a small value makes a small list cross chunk boundaries), "variant_lds_bytes" (LDS for the tables of one motif group
 * of those calls, 0 = the default of 24 576: a small value sends small motifs to the kernel that reads global memory),
 * "tally_launches" (1 = count the registry rows launched, lm_hip_ctx_launch_tally), "track_fold_cells" (score_into on handles
 * stores + tracks the maximum in ONE launch below this many cells and with block maxima + two reduction launches from it on;
 * default 8 Mi, 0 = always the latter: lets a small input take the large inputs' route); "xcd_remap" is accepted and ignored (the remap it selected was removed in round 5).  Unknown names:
 * LM_HIP_ERR_BAD_ARGS.  The shipped library reads none of them from the environment. */
int lm_hip_ctx_set_option(lm_hip_ctx *ctx, const char *name, double value);
/* Round-4 ABI: selected an XCD-aware workgroup remap of the store kernel, which measured slower and was removed in round 5.
 * Kept as a no-op returning LM_HIP_OK so that embedders built against the round-4 header still load and link. */
int lm_hip_ctx_set_xcd_remap(lm_hip_ctx *ctx, int enabled);
/* Name of the kernel the last score call on this context launched
 * (for profiling tools); valid until the next call.  "score_c32<M,MODE>" names
 * the kernel family and the length it ran at (MODE 0 store, 1 fused argmax,
 * 2 fused threshold); the store kernel's tracking forms (lm_hip_ctx_set_track_argmax:
 * template modes 3 and 5 in a rocprofv3 trace) report as "score_c32<M,0>". */
const char *lm_hip_ctx_last_kernel(lm_hip_ctx *ctx);
/* Diagnostic: rows per stream (T) of the last plain store launch on this context (score_into without the tracked
 * maximum) when ONE C = 32 store kernel carried it; 0 when it took another route, motifs stored in slices (more than
 * 36 rows) included.  Lengths whose kernel stores score
 * rows in pairs always report an even number (lm_hip_ctx_set_rows_per_stream rounds to the nearest such length). */
unsigned long long lm_hip_ctx_last_stream_rows(lm_hip_ctx *ctx);
/* Diagnostic: what the last fused threshold scan on this context (single or batched) produced -- hits, and CANDIDATES: the
 * pieces of up to 32 rows the discrete prefilter flagged for exact re-scoring.  Candidates per hit is how much a
 * sequence costs beyond the scan itself (low-complexity tracts and N runs raise it: profiles/r05_realistic_inputs.json).
 * Either output may be NULL. */
int lm_hip_ctx_last_scan_counts(lm_hip_ctx *ctx, unsigned long long *hits, unsigned long long *candidates);
/* Diagnostic: with the context option "time_scan" = 1, the duration (ms, HIP events on the context's stream) of the scan
 * kernel(s) of the last fused threshold / fused argmax call -- the part of the call that the LDS roofline bounds, without
 * the re-scoring, the ordering of the hit list and the read-back behind it (bench.py: roofline.kernel_frac of the fused
 * blocks).  -1 when the option is off or the call took a route without a scan kernel. */
int lm_hip_ctx_last_scan_kernel_ms(lm_hip_ctx *ctx, float *ms);
/* Diagnostic ("time_scan" = 1): the last fused THRESHOLD call (single or batched) by phase, in ms -- [0] the scan kernels,
 * [1] the exact re-scoring of their candidates, [2] the kernels that order the hit list (HIP events on the context's
 * stream), [3] the rest of the call on the host clock: enqueueing, the synchronisation's wake-up, the copy of the results
 * out of the pinned block.  -1 where nothing was recorded.  After lm_hip_seq_count_symbols / lm_hip_seqset_count_symbols:
 * [0] the block pass, [1] the scan of its table, [2] the prefix pass and the differences, [3] -1. */
int lm_hip_ctx_last_phases_ms(lm_hip_ctx *ctx, float phases[4]);
/* Diagnostic: what the scan kernel of the last SINGLE-job fused call on this context looked up per position -- the motif
 * rows it scanned (a pair scan of M = 20, 24, ... 36 may look M - 1 rows up and credit the last one with its best weight)
 * and the bytes of LDS table that costs (what a roofline figure must be priced against).  Zeros: no such scan ran (a batch,
 * an argmax settled from the last rows, a chunked route).  Either pointer may be NULL. */
int lm_hip_ctx_last_scan_info(lm_hip_ctx *ctx, size_t *motif_rows_scanned, size_t *lds_bytes_per_position);
/* One row of the library's registry of unrolled kernels: a kernel family, the alphabet width it is built for (1 = more than
 * 16 symbols), the motif length M it is instantiated at and, for LM_HIP_FAMILY_C32, its slot (0 store with byte symbol loads,
 * 1 fused argmax, 2 fused threshold, 3 store with dword symbol loads, 4 store + block maxima, 5 continue in place, 6 store at
 * 16 columns, 7 store + tracked maximum; 0 for every other family). */
typedef struct lm_hip_registry_row {
    int family, wide, m, slot;
    unsigned long long value; /* lm_hip_ctx_launch_tally: launches; lm_hip_registry_rows: equal for rows that share one kernel */
} lm_hip_registry_row;
#define LM_HIP_FAMILY_C32 0          /* exact f32 kernels, score_c32<M, MODE> */
#define LM_HIP_FAMILY_PRE 1          /* one-symbol prefilter scan */
#define LM_HIP_FAMILY_PREBLK 2       /* ... on 4-row symbol blocks (protein) */
#define LM_HIP_FAMILY_PRE2 3         /* DNA pair scan */
#define LM_HIP_FAMILY_PRE2_PROTEIN 4 /* pair scan over the 441 residue pairs */
#define LM_HIP_FAMILY_PRE2_MULTI 5   /* DNA pair scan, several motifs per pass */
#define LM_HIP_FAMILY_U8 6           /* u8 scores of a DiscreteMatrix, one symbol per lookup */
#define LM_HIP_FAMILY_U8_PAIRS 7     /* ... two symbols per lookup (DNA) */
#define LM_HIP_FAMILY_BEST_FUSED 8   /* best hit per record of a sequence set */
/* Diagnostic: every row the build registered (the non-null cells of the registry's tables and of the table of
 * lm_hip_scan_best_seqset, read from the tables themselves).  Writes at most `cap` rows, *count = the number there are.  Host
 * only: needs no device. */
int lm_hip_registry_rows(lm_hip_registry_row *rows, size_t cap, size_t *count);
/* Diagnostic: with the context option "tally_launches" = 1, the registry rows this context has LAUNCHED since the last call
 * (counted where a kernel is enqueued, not where a row is looked up), `value` = launches.  Writes at most `cap` rows,
 * *count = the number there are; the tally is cleared when all of them fit (cap >= *count).  Option off: *count = 0. */
int lm_hip_ctx_launch_tally(lm_hip_ctx *ctx, lm_hip_registry_row *rows, size_t cap, size_t *count);

/* ---- PSSM ---------------------------------------------------------------- */

/* ScoringMatrix<A>.matrix() (pwm/mod.rs:561-564): `pssm` = pssm[0].as_ptr(),
 * m = rows(), stride = stride() (8 for Dna, 24 for Protein), k = A::K::USIZE.
 * Columns >= k of a row are never read (A4: they may be uninitialised). */
int lm_hip_pssm_create(lm_hip_ctx *ctx, const float *pssm, size_t m, size_t stride,
                       size_t k, lm_hip_pssm **out);
int lm_hip_pssm_destroy(lm_hip_pssm *pssm);
size_t lm_hip_pssm_len(const lm_hip_pssm *pssm);

/* ScoringMatrix::<Dna>::reverse_complement (pwm/mod.rs:566-577): a new resident matrix with
 * rows reversed and the columns of complementary nucleotides swapped (A<->T, C<->G, N kept;
 * abc.rs Dna::complement) -- the second strand of `lightmotif-cli --reverse` (main.rs) without
 * a host round trip.  DNA matrices (k == 5) only: LM_HIP_ERR_BAD_ARGS otherwise. */
int lm_hip_pssm_reverse_complement(lm_hip_ctx *ctx, const lm_hip_pssm *pssm, lm_hip_pssm **out);

/* ---- Score (device pointers) ---------------------------------------------- */

/*
 * Score::score_rows_into (pli/mod.rs:72-106) / Avx2::score_f32_rows_into
 * (avx2.rs:889-904).
 *   d_seq            seq.matrix()[0].as_ptr(), on the device
 *   seq_rows_total   seq.matrix().rows()   (includes the wrap rows)
 *   seq_stride       seq.matrix().stride()
 *   cols             C (32 through pssm.score() on x86-64, dispatch.rs:45)
 *   wrap, length     seq.wrap(), seq.len()
 *   [row_begin,row_end)  the `rows` range
 *   d_out            scores.matrix_mut()[0].as_mut_ptr(), on the device, with
 *                    room for (row_end-row_begin) rows of out_stride floats
 * On return *out_rows / *max_index hold the arguments the reference passes to
 * scores.resize (pli/mod.rs:86,91): (0,0) in the degenerate case, else
 * (row_end-row_begin, L+1-M).  Asynchronous on the context's stream.
 * Errors: LM_HIP_ERR_WRAP if wrap < M-1; BAD_ARGS if row_end > rows.
 */
int lm_hip_score_f32_dptr(lm_hip_ctx *ctx, const lm_hip_pssm *pssm,
                          const uint8_t *d_seq, size_t seq_rows_total, size_t seq_stride,
                          size_t cols, size_t wrap, size_t length,
                          size_t row_begin, size_t row_end,
                          float *d_out, size_t out_stride,
                          size_t *out_rows, size_t *max_index);

/* ---- Maximum / Threshold (device pointers) -------------------------------- */

/* Maximum::argmax, Generic semantics (pli/mod.rs:135-155): the maximal cell
 * that is LAST in (row, col) order; NaN never wins; if scores[0][0] is NaN the
 * answer is (0,0).  *found = 0 when rows == 0.  `value` (optional) receives
 * Maximum::max (pli/mod.rs:158-160).  Synchronises. */
int lm_hip_argmax_f32_dptr(lm_hip_ctx *ctx, const float *d_scores, size_t rows,
                           size_t stride, size_t cols, int *found,
                           lm_hip_coords *best, float *value);
/* Maximum::max (pli/mod.rs:158-160) on its own: the value AT that argmax -- NaN when
 * scores[0][0] is NaN, -inf for an all -inf matrix; *found = 0 (None) when rows == 0.
 * (NOT Avx2::max_f32, which seeds with 0.0: avx2.rs:438-441.) */
int lm_hip_max_f32_dptr(lm_hip_ctx *ctx, const float *d_scores, size_t rows, size_t stride,
                        size_t cols, int *found, float *value);

/* Same for one SHARD of a row-partitioned score matrix (multi-GPU):
 * with first_cell_rule = 0 the "scores[0][0] is NaN -> (0,0)" rule is not applied,
 * because the shard's first cell is not the matrix's first cell; the caller
 * applies it once, on the shard that holds row 0.  first_cell_rule = 1 is
 * lm_hip_argmax_f32_dptr. */
int lm_hip_argmax_shard_f32_dptr(lm_hip_ctx *ctx, const float *d_scores, size_t rows,
                                 size_t stride, size_t cols, int first_cell_rule, int *found,
                                 lm_hip_coords *best, float *value);

/* Threshold::threshold (pli/mod.rs:210-221): every (row, col) with x >= t, in
 * row-major order (the reference's push order).  *coords is malloc'ed by the
 * library (NULL when *n == 0); release with lm_hip_free.  Synchronises. */
int lm_hip_threshold_f32_dptr(lm_hip_ctx *ctx, const float *d_scores, size_t rows,
                              size_t stride, size_t cols, float t,
                              lm_hip_coords **coords, size_t *n);

/* ---- Score / Maximum / Threshold on u8 (DiscreteMatrix scores) ------------- */

/* Score<u8, A, C>::score_rows_into with the weights of a DiscreteMatrix
 * (pwm/mod.rs:754-791; what Scanner::next scores first, scan.rs:174-178).
 *   weights          dm.matrix()[0].as_ptr() ON THE HOST: m rows of weights_stride bytes,
 *                    k = A::K used per row (DenseMatrix<u8, K>; 400 bytes at most, copied per call)
 *   d_seq .. row_end as lm_hip_score_f32_dptr
 *   d_out            u8 scores on the device, (row_end-row_begin) rows of out_stride bytes
 *   saturate         1: the saturating byte adds of the SIMD back-ends (avx2.rs:336
 *                    `_mm256_adds_epu8`; what `dispatch` runs on x86-64) -> min(sum, 255);
 *                    0: Generic's `+=` on u8 (pli/mod.rs:98-102, wrapping in release
 *                    builds) -> sum mod 256.  They agree whenever no sum exceeds 255.
 * Same pre-checks, degenerate cases and *out_rows / *max_index as the f32 form.
 * Asynchronous on the context's stream. */
int lm_hip_score_u8_dptr(lm_hip_ctx *ctx, const uint8_t *weights, size_t m, size_t weights_stride,
                         size_t k, const uint8_t *d_seq, size_t seq_rows_total, size_t seq_stride,
                         size_t cols, size_t wrap, size_t length, size_t row_begin, size_t row_end,
                         uint8_t *d_out, size_t out_stride, int saturate,
                         size_t *out_rows, size_t *max_index);

/* The same on a resident sequence handle, scores returned to the HOST: `out` receives
 * (row_end-row_begin) rows of out_stride bytes (`cols` written per row), i.e. the
 * StripedScores<u8, C> matrix a Rust caller owns (scores.matrix_mut()[0].as_mut_ptr()).
 * Synchronises. */
int lm_hip_score_u8(lm_hip_ctx *ctx, const uint8_t *weights, size_t m, size_t weights_stride,
                    size_t k, const lm_hip_seq *seq, size_t row_begin, size_t row_end, int saturate,
                    uint8_t *out, size_t out_stride, size_t *out_rows, size_t *max_index);

/* Maximum<u8, C>::argmax / max, Generic semantics (pli/mod.rs:135-160; scan.rs:181 takes
 * `max`): the maximal cell that is LAST in (row, col) order.  Synchronises. */
int lm_hip_argmax_u8_dptr(lm_hip_ctx *ctx, const uint8_t *d_scores, size_t rows, size_t stride,
                          size_t cols, int *found, lm_hip_coords *best, uint8_t *value);

/* Threshold<u8, C>::threshold (pli/mod.rs:210-221; scan.rs:184): every (row, col) with
 * x >= t in row-major order; *coords malloc'ed, release with lm_hip_free.  Synchronises. */
int lm_hip_threshold_u8_dptr(lm_hip_ctx *ctx, const uint8_t *d_scores, size_t rows, size_t stride,
                             size_t cols, uint8_t t, lm_hip_coords **coords, size_t *n);

/* ---- fused score + reduce (no score matrix is written) -------------------- */

/* Equivalent to score_rows_into followed by argmax on the result
 * (lightmotif-bench/dna.rs:104-107 times exactly that pair).  `best` is in the
 * coordinates of the scored block (row relative to row_begin).  *found = 0 in
 * the degenerate case. */
int lm_hip_score_argmax_f32_dptr(lm_hip_ctx *ctx, const lm_hip_pssm *pssm,
                                 const uint8_t *d_seq, size_t seq_rows_total,
                                 size_t seq_stride, size_t cols, size_t wrap, size_t length,
                                 size_t row_begin, size_t row_end,
                                 int *found, lm_hip_coords *best, float *value);

/* Shard form of the fused argmax (see lm_hip_argmax_shard_f32_dptr). */
int lm_hip_score_argmax_shard_f32_dptr(lm_hip_ctx *ctx, const lm_hip_pssm *pssm,
                                       const uint8_t *d_seq, size_t seq_rows_total,
                                       size_t seq_stride, size_t cols, size_t wrap, size_t length,
                                       size_t row_begin, size_t row_end, int first_cell_rule,
                                       int *found, lm_hip_coords *best, float *value);

/* Equivalent to score_rows_into followed by threshold(t): (row, col) list in
 * row-major order, rows relative to row_begin. */
int lm_hip_score_threshold_f32_dptr(lm_hip_ctx *ctx, const lm_hip_pssm *pssm,
                                    const uint8_t *d_seq, size_t seq_rows_total,
                                    size_t seq_stride, size_t cols, size_t wrap, size_t length,
                                    size_t row_begin, size_t row_end, float t,
                                    lm_hip_coords **coords, float **values, size_t *n);

/* ---- many motifs x one resident sequence ---------------------------------- */

/* lightmotif-cli sends every motif against every sequence (main.rs:554-561), one
 * Scanner per (motif, sequence) job.  These run `n` motifs over one resident
 * sequence as back-to-back fused kernels with a single synchronisation; no score
 * matrix is written.  The sequence must have wrap >= max(M) - 1 (the CLI does
 * configure_wrap(max_m), main.rs:540-546).  Per motif the results equal
 * score_into + argmax / threshold on the full row range.
 *   found/best/value : arrays of n
 *   counts           : array of n; *coords / *values hold sum(counts) entries,
 *                      motif after motif, each motif's hits in row-major order;
 *                      release both with lm_hip_free (NULL when there are no hits). */
int lm_hip_scan_argmax_batch(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n,
                             const lm_hip_seq *seq, int *found, lm_hip_coords *best, float *value);
int lm_hip_scan_threshold_batch(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms,
                                const float *thresholds, size_t n, const lm_hip_seq *seq,
                                size_t *counts, lm_hip_coords **coords, float **values);

/* ---- many motifs x many resident sequences --------------------------------- */

/* The other axis of the CLI's job product (main.rs:502-561: one job per (motif, record) pair): a SET of records --
 * a peak set, promoters, contigs -- resident as ONE striped sequence, so that the per-call costs (upload, stripe,
 * synchronisation, read-back) are paid once per set instead of once per record.  The records are laid end to end
 * WITHOUT separators: the matrix is exactly StripedSequence of the joined text (seq.rs:288-313), and since a score is
 * M sequential f32 adds over symbols p .. p+M-1 (pli/mod.rs:72-106) every window inside one record scores bit for
 * bit as it does when the record is striped alone.
 *   text / encoded   `total` bytes: ASCII (alphabet 'D' / 'P', strict or lossy as lm_hip_seq_from_ascii) or symbol
 *                    bytes < k (as lm_hip_seq_from_encoded); one upload, encode + stripe on the device
 *   offsets          n_records + 1 entries: record r is [offsets[r], offsets[r+1]); offsets[0] == 0, non-decreasing
 *                    (empty records are fine), offsets[n_records] == total -- LM_HIP_ERR_BAD_ARGS otherwise, checked
 *                    before any device work.  The table is kept on the device next to the matrix, 64-bit entries.
 *   bad_record / bad_index   strict mode: the first invalid byte as (record, index inside the record) with
 *                    LM_HIP_ERR_INVALID_SYMBOL; either may be NULL
 * LM_HIP_ERR_CAPACITY when ceil(total / cols) * cols exceeds the 2^40 cells a hit list addresses, LM_HIP_ERR_OOM when
 * the device cannot hold the matrix. */
int lm_hip_seqset_from_ascii(lm_hip_ctx *ctx, char alphabet, const uint8_t *text, size_t total,
                             const uint64_t *offsets, size_t n_records, size_t cols, int lossy,
                             lm_hip_seqset **out, size_t *bad_record, size_t *bad_index);
int lm_hip_seqset_from_encoded(lm_hip_ctx *ctx, const uint8_t *encoded, size_t total,
                               const uint64_t *offsets, size_t n_records, size_t cols, size_t k,
                               lm_hip_seqset **out);
/* StripedSequence::configure_wrap (seq.rs:369-381) on the set's matrix (the CLI: configure_wrap(max_m), main.rs:540-546). */
int lm_hip_seqset_configure_wrap(lm_hip_ctx *ctx, lm_hip_seqset *set, size_t m);
/* records, len() of the concatenation, matrix().rows() - wrap(), wrap(), cols, alphabet size; any pointer may be NULL. */
int lm_hip_seqset_info(const lm_hip_seqset *set, size_t *records, size_t *total_length, size_t *rows,
                       size_t *wrap, size_t *cols, size_t *k);
int lm_hip_seqset_record_length(const lm_hip_seqset *set, size_t record, size_t *length);
/* All record lengths at once; LM_HIP_ERR_CAPACITY when `capacity` < records. */
int lm_hip_seqset_lengths(const lm_hip_seqset *set, size_t *lengths, size_t capacity);
int lm_hip_seqset_destroy(lm_hip_seqset *set);

/* A set straight from the bytes of a FASTA file: the reference CLI's compiled reader in front of encode_lossy
 * (main.rs:532-546, seq.rs:122-129), with the container parsed ON THE DEVICE (csrc/fasta.hip) -- the host uploads the
 * raw bytes and never looks at a sequence line.  The grammar, on bytes: lines end at '\n' (the last need not have one); a
 * line whose first byte is '>' is a header line and starts a record; every other line is a sequence line of the record
 * opened by the nearest header line before it, and sequence lines before the first header are dropped; in sequence lines
 * the bytes 0x09-0x0D and 0x20 are dropped wherever they stand and every other byte is a residue that goes through the
 * table of lm_hip_seq_from_ascii (a '>' in mid-line is an invalid residue); records may be empty, and input without a
 * header line is a set of zero records.  For plain FASTA (ASCII, "\n" or "\r\n" line ends, whitespace only at the ends of
 * a sequence line) these are the records a line-by-line text reader yields; they differ on whitespace inside a sequence
 * line (dropped here), on a lone '\r' (no line end here) and on non-ASCII bytes (invalid residues here).
 *   out        an ordinary lm_hip_seqset: matrix and offsets equal, byte for byte, what lm_hip_seqset_from_ascii
 *              builds from the parsed records
 *   headers    may be NULL; otherwise *headers receives *n_records spans (NULL when there are none; release with
 *              lm_hip_free): bytes [begin, end) of `text` = one header line without its '>' and without its '\n' (a
 *              '\r' in front of the '\n' stays inside the span)
 *   bad_record / bad_index   strict mode, LM_HIP_ERR_INVALID_SYMBOL: the first offending residue (the smallest position
 *              of the concatenation) as (record, index inside the record), as lm_hip_seqset_from_ascii; either may be NULL
 * LM_HIP_ERR_BAD_ARGS, before any device work, for a null ctx / out / n_records, a null text with nbytes > 0, cols == 0 or
 * an alphabet other than 'D' / 'P'; LM_HIP_ERR_CAPACITY when the residues exceed the 2^40 cells a hit list addresses;
 * LM_HIP_ERR_OOM as lm_hip_seqset_from_ascii.  On any failure *out is NULL.  Device memory peaks below 3 x nbytes (raw
 * text, compact text, matrix); the first two are released before the call returns.  Every position and count is 64-bit;
 * results are identical from call to call.  Synchronises. */
typedef struct { uint64_t begin, end; } lm_hip_fasta_span;   /* bytes [begin, end) of the input */
int lm_hip_seqset_from_fasta(lm_hip_ctx *ctx, char alphabet, const uint8_t *text, size_t nbytes,
                             size_t cols, int lossy, lm_hip_seqset **out,
                             lm_hip_fasta_span **headers, size_t *n_records,
                             size_t *bad_record, size_t *bad_index);
/* Bytes of input one workgroup parses (the tile of csrc/fasta.hip); needs no device. */
size_t lm_hip_fasta_tile_bytes(void);

/* `n` motifs x every record of the set in ONE call (main.rs:502-561 collapsed): per motif, in caller order, every
 * (record, position) with score >= threshold and position + M <= len(record) (scan.rs:185-190, per RECORD), sorted by
 * record, then position.  counts[i] hits for motif i; *hits holds sum(counts) entries (release with lm_hip_free; NULL
 * when there are none).  Scores and hit sets equal, bit for bit, lm_hip_scan_threshold_batch + that cut on each record
 * striped alone; NaN / -inf thresholds and weights behave as there.  The scans are those of
 * lm_hip_scan_threshold_batch over the concatenation; windows that straddle two records or run past a record's end
 * are dropped, and positions made record-relative, by a segment pass on the device (csrc/seqset.hip) before anything
 * is read back.  LM_HIP_ERR_WRAP when the set's wrap < max(M) - 1; LM_HIP_ERR_BAD_ARGS, before any launch, when a
 * matrix's alphabet size differs from the set's.  A motif longer than every record has no hits. */
int lm_hip_scan_threshold_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds,
                                 size_t n, const lm_hip_seqset *set, size_t *counts, lm_hip_set_hit **hits);

/* The dense motifs x records matrix of best windows: what the reference's README asks of one sequence
 * (`pssm.score(&striped).argmax()`, scores.rs:190-192) and its CLI would ask once per (motif, record) job
 * (main.rs:502-561), for every motif and every record of the set in ONE call, without a score matrix or a hit list.
 * best[i * records + r] (motif-major, caller's memory, n * records entries) describes motif i (M rows) in record r
 * (L_r symbols).  The windows are the positions p = 0 .. L_r - M, all inside the record (scan.rs:185-190, per RECORD);
 * each scores as score_into scores it, M sequential f32 adds from +0.0 in row order (pli/mod.rs:96-105), bit for bit
 * the score it has when the record is striped alone.
 *   found = 0   the record has no window (L_r < M, empty records included) or every window scores NaN;
 *               then position = 0 and score = NaN
 *   found = 1   score = the greatest window score under f32 `>` (NaN windows never compete, -inf windows do: a record
 *               of only -inf windows answers (-inf, 0)), position = the LOWEST record-relative position holding it
 * i.e. among record r's hits in lm_hip_scan_threshold_seqset's list for a threshold of -inf, the greatest score and
 * the first of those in list order.  Deterministic, identical from call to call and with the prefilter on or off: the
 * route is exact f32 throughout (csrc/seqset_best.hip on the record walk of csrc/seqset_walk.hpp;
 * lm_hip_ctx_last_kernel names the kernel that ran last, `seqset_best_fused<M>` up to M = 36, `seqset_best_generic`
 * beyond).
 * This deliberately is NOT Maximum::argmax (pli/mod.rs:135-155) on the record's own score matrix: that rule also scans
 * the cells of the padded tail and takes the LAST maximal cell in (row, col) order.  The two agree -- same score, and
 * position = col * rows + row of the record striped alone -- when the maximum over the valid windows is unique and the
 * default symbol's column of the matrix is -inf (no padded cell can then reach it).
 * LM_HIP_ERR_WRAP when the set's wrap < max(M) - 1; LM_HIP_ERR_BAD_ARGS, before any launch, on null arguments or a
 * matrix whose alphabet size differs from the set's; LM_HIP_OK with nothing written when n == 0 or the set has no
 * records; LM_HIP_ERR_OOM when the device cannot hold the result block of one motif (motifs are scanned in groups that
 * bound the block at 256 MB).  The merge packs record-relative positions into 32 bits: a set with a record of 2^32 or
 * more symbols is refused with LM_HIP_ERR_CAPACITY before any launch; offsets and global positions are 64-bit
 * throughout. */
int lm_hip_scan_best_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const lm_hip_seqset *set,
                            lm_hip_set_best *best);

/* How many windows of every motif reach a cut-off in every record of the set, at up to LM_HIP_MAX_COUNT_LEVELS cut-offs
 * per motif, in ONE call and without a hit list: the count the reference's CLI would reach by collecting the hits of
 * every (motif, record) job (main.rs:502-561) and counting them per record.
 *   thresholds   thresholds[i * levels + l] is cut-off l of motif i, 1 <= levels <= LM_HIP_MAX_COUNT_LEVELS; several
 *                cut-offs of one motif cost one walk over the set
 *   counts       counts[(i * levels + l) * records + r], the caller's memory (n * levels * records cells); every cell is
 *                written, zeros included
 * A cell holds the number of positions p = 0 .. L_r - M of record r (all inside the record: scan.rs:185-190, per RECORD)
 * whose window score v satisfies v >= t under f32 comparison, v being the score score_into gives: M sequential f32 adds
 * from +0.0 in row order (pli/mod.rs:96-105), bit for bit the score of the record striped alone.  NaN windows are never
 * counted, -inf windows only when t is -inf, a NaN threshold counts nothing; windows that straddle two records or reach
 * the padding are never counted.  For every threshold value a cell equals the number of entries with that record in
 * lm_hip_scan_threshold_seqset's list for motif i at t.  A motif with no window anywhere (no rows, or longer than the
 * sequence) gives zeros.
 * Deterministic, identical from call to call and with the prefilter on or off: the route is exact f32 throughout and its
 * merge is a sum of integers (csrc/seqset_count.hip: the record walk of csrc/seqset_walk.hpp with per-lane counters
 * that reach the cells through 32-bit atomic adds; lm_hip_ctx_last_kernel names `seqset_count_fused<M>` up to M = 36,
 * `seqset_count_generic` beyond).
 * Measured on one MI355X (tools/seqset_bench.py --count, profiles/seqset_count_bench.json; 2 000 records x 500 bp x 8
 * JASPAR motifs, the set resident, medians of 15 alternating runs), against lm_hip_scan_threshold_seqset at the same
 * thresholds plus one count per motif on the host, the cheapest way before: 0.135 ms against 2.14 ms at p = 1e-1 (768 000
 * hits, 15.8 x), 0.118 against 0.345 ms at 1e-2 (2.9 x), 0.111 against 0.162 ms at 1e-3 (1.5 x); at 1e-4 and 1e-5 the two
 * are level within the spread between runs (list / count = 1.18 and 1.18 in one run, 1.04 and 0.96 in its repeat), so the
 * crossover lies at about p = 1e-5 and from there down the list route, which also says WHERE the hits are, stays the
 * right call.  Three cut-offs (1e-1, 1e-2, 1e-3) in one call: 0.143 ms against 4.19 ms for the list at 1e-1 plus three
 * counts (29 x).  The same call of lm_hip_scan_best_seqset, the same walk, takes 0.131-0.135 ms: counting costs 0.83-1.0 x
 * the best hit (4-byte cells, no finalize kernel).
 * LM_HIP_ERR_WRAP when the set's wrap < max(M) - 1; LM_HIP_ERR_BAD_ARGS, before any launch, on null arguments (with
 * n > 0 a null `thresholds`, and a null `counts` when the set has records), `levels` of 0 or above
 * LM_HIP_MAX_COUNT_LEVELS, or a matrix whose alphabet size differs from the set's; LM_HIP_OK with nothing written when
 * n == 0 or the set has no records; LM_HIP_ERR_CAPACITY, before any launch, when a record holds 2^32 or more symbols (a
 * cell is 32 bits); LM_HIP_ERR_OOM when the device cannot hold the cells of one motif (motifs are scanned in groups that
 * bound the block at 256 MB). */
#define LM_HIP_MAX_COUNT_LEVELS 4
int lm_hip_scan_count_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds,
                             size_t levels, size_t n, const lm_hip_seqset *set, uint32_t *counts);

/* The total odds of every motif in every record of the set, in ONE call and without a hit list: with the best window
 * ("max odds") and the hit count ("total hits") the statistic motif-enrichment tools call "sum odds" -- and, over the
 * number of windows, "average odds" --, the affinity of a record for a factor.  For motif i (M rows, scale s_i) and record
 * r (L_r symbols)
 *       sums[i * records + r] = sum over p = 0 .. L_r - M, v_p not NaN, of 2^( fl32(s_i * v_p) )          (a double)
 *   v_p       the window score exactly as score_into gives it: M sequential f32 adds from +0.0 in row order
 *             (pli/mod.rs:96-105), bit for bit the score lm_hip_scan_best_seqset and lm_hip_scan_count_seqset see
 *   scales    n of them, or NULL: all 1.  s_i * v_p is ONE f32 multiply, exact for s_i == 1 (a log2-odds matrix); other
 *             scales serve matrices in another base (s = log2(base)) or a temperature
 *   sums      the caller's memory, n * records doubles; every cell is written
 * Windows that straddle two records or reach the padding never contribute (scan.rs:185-190, per RECORD); NaN windows
 * contribute nothing, the rule of best and count; -inf windows contribute 0; a +inf window makes the cell +inf.  A record
 * with no window gives 0.0 and a motif with no window anywhere (no rows, or longer than the sequence) a row of zeros.
 * The exponential neither overflows nor flushes to zero while the value is a double: x = s * v is split into rint(x) and
 * an exact f32 fraction in [-1/2, 1/2], the fraction goes through the hardware's f32 exp2 (1 ulp), the result is widened
 * and scaled by 2^rint(x) in f64 (|x| is clamped at 2 000, where a double is +inf or 0 either way).  A term is therefore
 * right to about 2^-23 relative, and a cell, a sum of positive terms added in f64, to the same.
 * Deterministic without a floating-point atomic: a record whose windows lie in one lane's run of the walk is stored by
 * that lane, the others are merged from per-run partial sums in ascending position order by a second kernel
 * (csrc/seqset_sum.hip, csrc/seqset_sum_plan.hpp, on the record walk of csrc/seqset_walk.hpp; lm_hip_ctx_last_kernel
 * names `seqset_sum_fused<M>` up to M = 36, `seqset_sum_generic` beyond).  Calls with the same context settings and the
 * same list of motifs give bit-identical tables.  The order of the f64 additions follows the cut of the set into lane runs,
 * so another rows_per_stream (or another number of motifs in the call, which moves the default) may change the last bits of
 * a cell: by no more than the f64 rounding of the additions, n * 2^-53 relative for n windows.
 * Measured on one MI355X (tools/seqset_bench.py --sum, profiles/seqset_sum_bench.json; 2 000 records x 500 bp x 8 JASPAR
 * motifs, the set resident, medians of 15 alternating runs): 0.288 ms against 39.4 ms for lm_hip_scan_threshold_seqset at
 * -inf plus exp2 and a sum per record on the host, the only way before (137 x); lm_hip_scan_count_seqset at one level, the
 * same walk with the cheapest reducer, takes 0.127 ms there (sum / count = 2.3 in that alternation, 1.09 in a series of
 * its own: DESIGN 4.6c.2) and 1.397 against 1.384 ms on 2 000 x 50 000 bp (sum / count = 0.99).  Worst relative
 * error of a cell against the f64 rule: 6.3e-08.
 * LM_HIP_ERR_WRAP when the set's wrap < max(M) - 1; LM_HIP_ERR_BAD_ARGS, before any launch, on null arguments (a null
 * `sums` when n > 0 and the set has records), a matrix whose alphabet size differs from the set's, or a scale that is not
 * finite or not > 0; LM_HIP_OK with nothing written when n == 0 or the set has no records; LM_HIP_ERR_OOM when the device
 * cannot hold the cells and partial sums of one motif (motifs are scanned in groups that bound the block at 256 MB).  The
 * cells are doubles: records of 2^32 symbols and more are served. */
int lm_hip_scan_sum_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *scales, size_t n,
                           const lm_hip_seqset *set, double *sums);

/* The expected site counts of every motif over the set, in ONE call: the E-step of motif EM (MEME's OOPS / ZOOPS), the
 * deterministic form of the sampler's step "score the record, weigh every window by 2^(score / temperature), rebuild the
 * count matrix" (sampler.rs:528-538 with CountMatrix::from_sequences, pwm/mod.rs:209-237; the windows of a RECORD as
 * scan.rs:185-190).  For motif i (M rows, scale s_i) a table of M x K doubles
 *       E[j][s] = sum over records r and windows p of z(r, p) * [symbol(r, p + j) == s]
 *   windows   of record r: the positions p with p + M <= len(r)
 *   v         the window score exactly as score_into gives it: M sequential f32 adds from +0.0 in row order, bit for bit
 *             the score lm_hip_scan_best_seqset, lm_hip_scan_count_seqset and lm_hip_scan_sum_seqset see
 *   e         exp2_wide(fl32(s_i * v)), the term of lm_hip_scan_sum_seqset (csrc/seqset_sum_plan.hpp)
 *   z         min(e * gains[i * records + r], 1.0) in f64: the posterior of the window.  A window whose score is NaN, or
 *             whose product e * gain is NaN (+inf * 0), contributes nothing; -inf scores give 0, +inf scores 1
 *   q         (u64) rint(z * 2^F), round to nearest even, F = min(40, 62 - bit_length(N)), N the positions of the set: F
 *             is a function of the set alone and no cell can overflow 64 bits (z <= 1, a cell sums at most N windows)
 *   Q[j][s]   the sum of q over the windows whose symbol at offset j is s: an exact integer;  E = (double) Q * 2^-F
 *   scales    n of them, or NULL: all 1 (1 / temperature), finite and > 0 as for lm_hip_scan_sum_seqset
 *   gains     n * records doubles, row-major, each finite and >= 0; gain 0 switches a record off.  1 / Z_r with Z the
 *             cell of lm_hip_scan_sum_seqset is the OOPS posterior
 *   counts    the caller's memory: the n tables of M_i x K doubles, row-major, one behind the other; K is the alphabet's
 *             size with its default symbol (5 / 21), as in a CountMatrix.  Every cell is written
 *   frac_bits NULL, or where F goes
 * Integer additions have no order, so the tables are a pure function of (set, matrix, scale, gains): the same bits from
 * run to run, at any rows_per_stream and with any number of motifs in the call; no floating-point atomic is used.  A
 * window with q == 0 is skipped, exactly.  Every row j of a motif's Q has the same total, the sum of q over its windows.
 * One kernel for every motif length (csrc/seqset_expect.hip on the record walk of csrc/seqset_walk.hpp;
 * lm_hip_ctx_last_kernel names `seqset_expect_generic`): a workgroup gathers its windows into a table of u64 counters in
 * LDS and adds the non-zero ones to Q with 64-bit integer atomics.  A motif with no window anywhere returns zeros.
 * LM_HIP_ERR_WRAP when the set's wrap < max(M) - 1; LM_HIP_ERR_BAD_ARGS, before any launch, on null arguments (null
 * `gains` or `counts` when n > 0 and the set has records), a matrix whose alphabet size differs from the set's, a scale
 * that is not finite or not > 0, or a gain that is NaN, infinite or negative; LM_HIP_OK with no table written when n == 0
 * or the set has no records. */
int lm_hip_seqset_expected_counts(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *scales,
                                  const double *gains, size_t n, const lm_hip_seqset *set, double *counts,
                                  int *frac_bits);

/* SymbolCount::count_symbols of a StripedSequence (seq.rs:444-483, the loop of seq.rs:466-482), and the same for every
 * record of a set in ONE call: what Background::from_sequence / from_sequences (abc.rs:404-456) count before
 * Background::from_counts (abc.rs:389-402) turns the table into frequencies, on the resident bytes (csrc/composition.hip).
 *   positions   position p of the sequence (of the concatenation, for a set) sits at row p % rows, column p / rows, with
 *               rows = matrix().rows() - wrap() = ceil(length / cols) (pli/mod.rs:178-200).  Exactly the positions
 *               p < length are counted: the cells of the padded tail are not, although they hold the default symbol, and
 *               neither are the wrap rows (seq.rs:469-477) -- the result is the same before and after configure_wrap
 *   sets        record r owns positions [offsets[r], offsets[r + 1]); an empty record gives a row of zeros, the sum of
 *               row r is the record's length and the sum of the table is total_length
 *   counts      the caller's memory, row-major: k entries for a sequence, counts[r * k + s] (records * k entries) for a
 *               set, k = the handle's alphabet size; `capacity` is in ELEMENTS, LM_HIP_ERR_CAPACITY with nothing written
 *               when it is short
 *   bytes >= k  (possible in an adopted matrix, or one written through its device pointer) are counted in no bin and
 *               index nothing; the sum of a row is then smaller than the length
 *   empty       zero records: LM_HIP_OK, nothing written; length == 0: LM_HIP_OK, zeros written; no launch either way
 * LM_HIP_ERR_BAD_ARGS, with a message and before any device work, for a null ctx, handle or counts, for a handle that
 * lives on another device than the context, and for an adopted matrix described as holding more symbols than its cells.
 * Every position and count is 64-bit; the result is identical from call to call.  Each call enqueues on the context's
 * stream and synchronises it; lm_hip_ctx_last_kernel names the counting kernel ("count_blocks") afterwards.
 * TEMPORARY DEVICE MEMORY, from the context's scratch (handed back above 2 GB like every other call's): a table of
 * 12 k / T bytes per position (T = 1024 rows per block, the option "count_tile_rows": 0.06 bytes per position for DNA,
 * 0.25 for protein) and 16 k bytes per record.  The pass reads 1 byte per position. */
int lm_hip_seq_count_symbols(lm_hip_ctx *ctx, const lm_hip_seq *seq, uint64_t *counts, size_t capacity);
int lm_hip_seqset_count_symbols(lm_hip_ctx *ctx, const lm_hip_seqset *set, uint64_t *counts, size_t capacity);

/* Symbols read back OUT of a resident set (csrc/sites.hip): the text of hit windows -- FIMO's `matched_sequence` -- the
 * count matrix of a motif's sites, whole records.  A set built from FASTA bytes never passed through the host, so these
 * are the only way to see what a hit matched without parsing the file a second time.
 *   sites       n motifs in caller order; counts[i] CONSECUTIVE sites belong to motif i.  The sites lie
 *               `site_stride_bytes` (>= 16) apart, each a `size_t record` at +0 and a `size_t position` at +8: the
 *               lm_hip_set_hit list of lm_hip_scan_threshold_seqset passes as it is with sizeof(lm_hip_set_hit) = 24,
 *               packed (record, position) pairs with 16.
 *   windows     a site names the window [position + shifts[i], position + shifts[i] + widths[i]) of its record;
 *               widths[i] >= 1, shifts may be NULL (all zero).  It is VALID when record < records, position + shift >= 0
 *               and position + shift + width <= the record's own length, evaluated without wrap-around for every 64-bit
 *               position and shift: a window never leaves its record.  An invalid site is not an error.
 *   reads       symbol q of the concatenation sits at row q % rows, column q / rows (pli/mod.rs:178-200), which is
 *               StripedSequence's Index (seq.rs:433-442); wrap rows are never read, so the result is the same before and
 *               after lm_hip_seqset_configure_wrap.
 * lm_hip_seqset_windows writes the widths[i] symbol bytes (indices < k, not ASCII) of every site, motif-major and then
 * in site order: sum(counts[i] * widths[i]) bytes; invalid sites read 0xFF.  valid (may be NULL) receives one byte per
 * site, 1 or 0.  One site per record with width = the record's length reads whole records back.
 * lm_hip_seqset_count_sites is CountMatrix::from_sequences (pwm/mod.rs:209-237) over the windows of each motif's valid
 * sites -- the motif table the Gibbs sampler builds from its start positions (sampler.rs:412-422) -- without the windows
 * leaving the device: tables holds k * sum(widths) entries, motif-major and then row-major, table_i[j][s] = the number of
 * valid sites of motif i whose j-th symbol is s; used (n entries, may be NULL) the number of valid sites, which is what
 * every row of table_i sums to.  For the sites of a reverse-complemented matrix the table of the forward motif is
 * CountMatrix::reverse_complement of the result (pwm/mod.rs:313-321: rows reversed, columns swapped), a host matter.
 * `capacity` is in elements (bytes / table entries): LM_HIP_ERR_CAPACITY when it is short, and nothing is written.
 * LM_HIP_ERR_BAD_ARGS, before any device work: null arguments (with n > 0: counts, widths, sites and the output), a width
 * of 0, a stride below 16, a set that lives on another device than the context.  n == 0 or no sites at all: LM_HIP_OK,
 * tables zero-filled, nothing launched.  Every position and count is 64-bit; integer adds commute, so a call repeats
 * byte for byte.  Both calls enqueue on the context's stream and synchronise it; lm_hip_ctx_last_kernel then names
 * "site_windows", or "site_counts_lds" (a workgroup counts a slice of one motif's sites in a private LDS table and adds
 * its non-zero counters with one 64-bit atomic each) or "site_counts_direct" (width * k beyond 12 287 counters: every
 * symbol adds to global memory).  TEMPORARY DEVICE MEMORY: sites are uploaded and processed in chunks of at most 256 MB of
 * sites (16 bytes each) plus, for the windows, their bytes -- a single window may exceed that on its own; the option
 * "site_chunk" caps the sites per chunk.  Motifs without sites or wider than the whole set never reach the device. */
int lm_hip_seqset_windows(lm_hip_ctx *ctx, const lm_hip_seqset *set, const size_t *counts, const size_t *widths,
                          const int64_t *shifts, size_t n, const void *sites, size_t site_stride_bytes,
                          uint8_t *symbols, size_t capacity, uint8_t *valid /* may be NULL */);
int lm_hip_seqset_count_sites(lm_hip_ctx *ctx, const lm_hip_seqset *set, const size_t *counts, const size_t *widths,
                              const int64_t *shifts, size_t n, const void *sites, size_t site_stride_bytes,
                              uint64_t *tables, size_t capacity, uint64_t *used /* n entries, may be NULL */);

/* What a single-symbol substitution does to the sites of every motif (csrc/variants.hip): does it create, destroy,
 * strengthen or weaken one?  The reference has no such call; the scores are its ScoringMatrix::score_position
 * (pwm/mod.rs:651-662) of the record and of the record with one symbol replaced.
 *   variants    (record r, position p inside the record, alt symbol a), `a` a symbol index, not ASCII.  VALID when
 *               r < records, p < L_r and a < k, evaluated on 64-bit values without wrap-around.  An invalid variant is not an
 *               error: every motif reports "none" on both sides for it and its ref_symbol reads 0xFF.
 *   windows     for motif i (M rows) the starts s = max(0, p - M + 1) ... min(p, L_r - M): all windows that lie inside the
 *               record and cover p; none when L_r < M
 *   ref side    the greatest window score under f32 `>`, each score M sequential f32 adds from +0.0 in row order
 *               (pli/mod.rs:96-105), bit for bit what lm_hip_scan_threshold_seqset reports for that window.  NaN windows
 *               never compete, -inf windows do, and among equal scores the LOWEST start wins (the rule of
 *               lm_hip_scan_best_seqset)
 *   alt side    the same rule over the same starts with the symbol at p replaced by a.  a equal to the resident symbol
 *               gives the ref side again, bit for bit; a = k - 1 (N / X) is an ordinary symbol
 *   effect      per side `score` and `back` = p - s (0 ... M - 1); with no window, or only NaN windows, score is a NaN and
 *               back = LM_HIP_VARIANT_NONE
 * Wrap rows are never read: the results are the same before and after lm_hip_seqset_configure_wrap and there is no
 * LM_HIP_ERR_WRAP case.  Both strands are obtained as everywhere else: pass reverse-complemented matrices as further
 * motifs.  Indels and multi-symbol substitutions are out of scope.
 * lm_hip_seqset_variant_effects writes the dense block effects[i * n_variants + v] (motif-major, n * n_variants entries of
 * the caller's memory) and, when ref_symbols is not NULL, the resident symbol of every variant (n_variants bytes).
 * lm_hip_seqset_variant_hits keeps, per motif i in caller order, the pairs with ref_score >= thresholds[i] or
 * alt_score >= thresholds[i] under f32 comparison -- a site on at least one allele; a none side never passes, a NaN
 * threshold keeps nothing, -inf keeps every pair with a non-NaN side.  The list is ordered by motif, then ascending variant
 * index; counts[i] entries belong to motif i; *hits (release with lm_hip_free; NULL when there are none) holds sum(counts)
 * entries that equal the dense form's cells bit for bit.  The dense block exists on the device alone, chunk by chunk, and is
 * compacted there in order: only kept entries cross to the host.
 * Both calls are deterministic and repeat byte for byte, enqueue on the context's stream and synchronise it, and keep the
 * caller's variant order (duplicates and unsorted input are fine).  lm_hip_ctx_last_kernel names "variant_effects" (the
 * tables of a group of motifs staged in LDS) or "variant_effects_global" (a motif whose table exceeds the LDS budget, read
 * from global memory) -- whichever ran last -- or "variant_gather" when no motif has a window anywhere.
 * LM_HIP_ERR_BAD_ARGS, before any device work and with a message: a null ctx or set (also when n == 0); with n > 0 a null
 * `pssms`, null outputs or `thresholds`; with n_variants > 0 a null `variants`; a matrix whose alphabet size differs from
 * the set's; a set on another device than the context.  LM_HIP_ERR_CAPACITY, before any launch, for a motif of 2^32 rows or
 * more.  n == 0 or n_variants == 0: LM_HIP_OK, nothing launched, counts zeroed and *hits = NULL.
 * TEMPORARY DEVICE MEMORY, from the context's scratch (handed back above 2 GB like every other call's): variants are
 * processed in chunks (option "variant_chunk") and motifs in batches so that one dense block stays within 256 MB, plus
 * 2 W + 32 bytes per variant of a chunk (W = the longest motif that fits a record); LM_HIP_ERR_OOM when one chunk cannot
 * be held. */
typedef struct lm_hip_variant {
    size_t record;
    size_t position;
    uint8_t alt;
} lm_hip_variant; /* 24 bytes */
typedef struct lm_hip_variant_effect {
    float ref_score, alt_score;
    uint32_t ref_back, alt_back;
} lm_hip_variant_effect; /* 16 bytes */
typedef struct lm_hip_variant_hit {
    uint64_t variant;
    lm_hip_variant_effect effect;
} lm_hip_variant_hit; /* 24 bytes */
#define LM_HIP_VARIANT_NONE 0xFFFFFFFFu
int lm_hip_seqset_variant_effects(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const lm_hip_seqset *set,
                                  const lm_hip_variant *variants, size_t n_variants, lm_hip_variant_effect *effects,
                                  uint8_t *ref_symbols /* n_variants, may be NULL */);
int lm_hip_seqset_variant_hits(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds, size_t n,
                               const lm_hip_seqset *set, const lm_hip_variant *variants, size_t n_variants, size_t *counts,
                               lm_hip_variant_hit **hits, uint8_t *ref_symbols /* n_variants, may be NULL */);

/* A sequence set cut out of a resident set, on the device (csrc/regions.hip, csrc/regions_plan.hpp): a genome is uploaded
 * once as a set of contigs, and every peak set, promoter set or variant neighbourhood -- a BED file of intervals -- becomes
 * a derived set that every set call above takes as it is, without the genome crossing to the host again.  The reference has
 * no such call; the result is the StripedSequence (seq.rs:288-313) of the extracted records laid end to end.
 *   regions     n regions in caller order; they may be unsorted, duplicated or overlapping, so the result may be larger
 *               than its source.  Record i of the result is region i: the result keeps n records and indices stay aligned
 *               with the caller's table.
 *   clipping    a region names [start, end) of source record `record` (BED: 0-based, half-open) and is clipped to the
 *               record: s = max(start, 0), e = min(end, L_record), compared on 64-bit values with no intermediate that can
 *               wrap.  record >= records, or s >= e after clipping (which includes start >= end), is not an error: the region
 *               gives an EMPTY record.
 *   taken       may be NULL; otherwise n entries: taken[i] = (s, e), and s == e == 0 for an empty region
 *   strand      0: the symbols [s, e) in source order.  1 (DNA sets only): the reverse complement -- symbol j of the record
 *               is the complement (abc.rs:174-185) of source symbol e - 1 - j, on bytes 0 <-> 2 and 1 <-> 3 (A <-> T,
 *               C <-> G); every other byte (N, and whatever an adopted matrix may hold) maps to itself.
 *   out         an ordinary lm_hip_seqset on the source's device, with the source's cols and k, and wrap 0: its matrix
 *               and offsets equal, byte for byte, what lm_hip_seqset_from_encoded builds from the same records extracted
 *               on the host
 *   reads       symbol q of the source's concatenation sits at row q % rows, column q / rows (pli/mod.rs:178-200); wrap
 *               rows of the source are never read, so the result is the same before and after
 *               lm_hip_seqset_configure_wrap(src)
 * LM_HIP_ERR_BAD_ARGS, before any device work and with a message: a null ctx, src or out; null regions with n > 0; a strand
 * other than 0 or 1; strand == 1 on a set whose alphabet is not DNA (k != 5); a set on another device than the context.
 * LM_HIP_ERR_CAPACITY when the result would exceed the 2^40 cells a hit list addresses; LM_HIP_ERR_OOM as
 * lm_hip_seqset_from_encoded.  On any failure *out is NULL.  n == 0: LM_HIP_OK, a set of zero records, nothing launched;
 * all regions empty: n empty records, nothing launched.  Deterministic: a call repeats byte for byte.  Enqueues on the
 * context's stream and synchronises it; lm_hip_ctx_last_kernel names "region_gather" afterwards (a lane gathers 16
 * consecutive bytes of the result's joined text, one byte per source row, and stores them at once; the stripe kernel of
 * lm_hip_seq_from_encoded then lays the text out).
 * TEMPORARY DEVICE MEMORY, from the context's scratch (free for the next call when this one returns, and handed back above
 * 2 GB like every other call's): the joined text of the result (its length) and 24 bytes per non-empty region.
 * COST: a source record is a column walk of the striped matrix, so every gathered byte reads a 32-byte sector.  That suits
 * region sets that cover a few percent of the source; a region set that tiles the whole source re-reads it about 32 times
 * through the cache (tools/regions_bench.py, profiles/regions_bench.json measure both). */
typedef struct lm_hip_region {
    size_t record;
    int64_t start;
    int64_t end;
    uint8_t strand;
} lm_hip_region; /* 32 bytes */
typedef struct lm_hip_region_span {
    uint64_t start, end;
} lm_hip_region_span;
int lm_hip_seqset_from_regions(lm_hip_ctx *ctx, const lm_hip_seqset *src, const lm_hip_region *regions, size_t n,
                               lm_hip_seqset **out, lm_hip_region_span *taken /* n entries, may be NULL */);

/* A NULL sequence set drawn on the device: EncodedSequence::sample / StripedSequence::sample (seq.rs:131-143,
 * seq.rs:315-328) for n_records records at once, from a Background (abc.rs:389-402) -- the control every enrichment question
 * needs, without a host generator and an upload.  Record r has lengths[r] symbols; K = 5 ('D') or 21 ('P').
 *   uniforms    u(seed, R, j), for position j of record number R = record_base + r (64 bits), is output word j & 3 of the
 *               Philox4x32-10 block (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds)
 *               with key (lo32(seed), hi32(seed)) and counter (lo32(j >> 2), lo32(R), hi32(R), hi32(j >> 2)).  A record's
 *               text depends on the seed, its number and its own model only -- not on other records, on cols or on how the
 *               call was launched -- and a longer record extends a shorter one.
 *   thresholds  of a frequency row f[0 .. K): c_s = the running f64 sum of (double)f[t], t = 0 .. s, in index order;
 *               T[s] = floor(c_s / c_{K-1} * 2^32) for s < K - 1; draw(T, u) = #{s < K - 1 : u >= T[s]}.  A symbol of
 *               frequency zero is never drawn.  A row is VALID when every entry is finite and >= 0 and the sum is > 0.
 *   order 0     transitions == NULL: x_j = draw(T_model(r), u(seed, R, j)); frequencies holds n_models rows of K, one for
 *               all records (n_models == 1) or one per record (n_models == n_records)
 *   order 1     transitions != NULL ('D' and n_models == 1 only): frequencies is the `initial` row, transitions K rows of K;
 *               x_0 = draw(T_initial, u_0), x_j = draw(T_row(x_{j-1}), u_j).  A transition row whose sum is 0 stands for
 *               `initial` (the N row of a chain fitted on N-free text).
 *   out         an ordinary lm_hip_seqset on the context's device with `cols` columns and wrap 0: its matrix and offsets
 *               equal, byte for byte, what lm_hip_seqset_from_encoded builds from the rule's records.  Empty records keep
 *               their index.
 * LM_HIP_ERR_BAD_ARGS, before any device work and with a message: a null ctx, out or frequencies; null lengths with
 * n_records > 0; cols == 0; an alphabet other than 'D' / 'P'; n_models neither 1 nor n_records; transitions with 'P' or with
 * n_models != 1; a model row that a non-empty record would use and that is not valid (the message names the record or the
 * row; a transition row is only looked at when a record holds two symbols).  LM_HIP_ERR_CAPACITY when the result would
 * exceed the 2^40 cells a hit list addresses; LM_HIP_ERR_OOM as lm_hip_seqset_from_encoded.  On any failure *out is NULL.
 * n_records == 0: a set of zero records; all records empty: n_records empty records; nothing is launched for either.
 * Enqueues on the context's stream and synchronises it; lm_hip_ctx_last_kernel names the draw kernel afterwards:
 * "sample_iid" (a lane draws 16 consecutive bytes of the joined text, four per Philox block, and stores them at once) or
 * "markov_emit" (order 1: the step of a position is a map of the 5 states, 15 bits; three launches in stream order compose
 * the maps per tile, scan the tiles in one workgroup and replay every lane's run from the symbol that enters it -- no
 * workgroup waits for another).  lm_hip_sample_tile_bytes: the text bytes one workgroup emits; needs no device.
 * TEMPORARY DEVICE MEMORY, from the context's scratch: the joined text (its length), 16 bytes per non-empty record, a
 * threshold row of 32 ('D') or 96 ('P') bytes per non-empty record with per-record models, 5 bytes per tile for order 1. */
int lm_hip_seqset_sample(lm_hip_ctx *ctx, char alphabet, const uint64_t *lengths, size_t n_records, const float *frequencies,
                         size_t n_models /* 1, or n_records (order 0 only) */,
                         const float *transitions /* NULL: order 0; else K*K, 'D' only */, uint64_t seed, uint64_t record_base,
                         size_t cols, lm_hip_seqset **out);
size_t lm_hip_sample_tile_bytes(void);

/* Adjacent-pair counts of a set, what a first-order chain is fitted from (the pair statistics behind a Background,
 * abc.rs:389-402, one order up): counts[a * k + b] = the number of positions p of the concatenation with p and p + 1 in the
 * same record, symbol a at p and symbol b at p + 1, summed over the set, u64.  Bytes >= k (an adopted matrix) count
 * nowhere, as in lm_hip_seqset_count_symbols.  Integer arithmetic throughout: a call repeats bit for bit.
 * LM_HIP_ERR_BAD_ARGS for a null argument or a set on another device; LM_HIP_ERR_CAPACITY when capacity < k * k.
 * lm_hip_ctx_last_kernel names "pair_blocks" afterwards (nothing is launched for a set of fewer than two symbols). */
int lm_hip_seqset_count_pairs(lm_hip_ctx *ctx, const lm_hip_seqset *set, uint64_t *counts, size_t capacity);

/* ScoreDistribution of n matrices at once (pwm/dist.rs:51-226, `ScoringMatrix::to_score_distribution`
 * pwm/mod.rs:698-705): what turns the CLI's `--pvalue` into thresholds (main.rs:479-489) and a hit's score into the
 * `pvalue` column (main.rs:335), built and queried on the device (csrc/dist.hip) instead of motif by motif, hit by hit on
 * the host.  Per matrix: the weights are discretised to 0 .. 1000 per row (dist.rs:133-161; by the host, in f64), the
 * rows are convolved into the distribution of the discretised score (dist.rs:164-191: per cell the terms
 * `old[t - s] * bg[a]` are added in symbol order, one f64 multiply and one f64 add each, never fused), and the
 * survival function is the sequential sum from the top, clamped at 1 (dist.rs:194-213).  Every number equals, bit for
 * bit, what lightmotif_amd/dist.py computes on the host, and a call repeats byte for byte.
 *   pssms        n resident matrices; alphabets may be mixed.  A NaN or +inf weight, or a matrix without a finite
 *                weight, is LM_HIP_ERR_BAD_ARGS before any launch (the reference panics there); -inf weights are the
 *                symbols a row cannot hold and are skipped (dist.rs:158-161)
 *   backgrounds  NULL, or n pointers, each NULL or to k_i f32 frequencies (widened to f64 as dist.rs:171 does); NULL
 *                stands for the uniform background of abc.rs:473-487 (1 / (K - 1), 0 for the default symbol)
 *   n == 0       a valid, empty object
 * MEMORY HELD until lm_hip_dists_destroy: 8 * (1000 * sum(M) + n) bytes of device memory for the survival functions
 * (about 177 MB for the 2 346 matrices of JASPAR 2024) and 40 bytes per matrix; _create holds up to 4 spare tables per
 * compute unit on top while it runs.  LM_HIP_ERR_OOM when they do not fit.
 * SYNCHRONISATION: _create, _sf, _scores and _pvalues each enqueue on the context's stream and synchronise it before
 * they return; _len, _info and _destroy touch no stream. */
int lm_hip_dists_create(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const float *const *backgrounds,
                        lm_hip_dists **out);
size_t lm_hip_dists_len(const lm_hip_dists *dists);
/* One matrix's parameters: rows M, `scale` and `offset` of the discretisation (dist.rs:154-155; both whole numbers),
 * min_score / max_score (the lowest index <= sf_len - 2 / the highest index >= 1 with mass, 0 where there is none:
 * dist.rs:197-213) and sf_len = 1000 M + 1.  Any out pointer may be NULL.  LM_HIP_ERR_BAD_ARGS for motif >= n. */
int lm_hip_dists_info(const lm_hip_dists *dists, size_t motif, size_t *rows, double *scale, double *offset, int64_t *min_score,
                      int64_t *max_score, size_t *sf_len);
/* Copies one survival function (sf_len f64) to dst; LM_HIP_ERR_CAPACITY when `capacity` (in elements) is short. */
int lm_hip_dists_sf(lm_hip_ctx *ctx, const lm_hip_dists *dists, size_t motif, double *dst, size_t capacity);
/* ScoreDistribution::score (dist.rs:104-116) of every matrix in one call: pvalues[i] -> scores[i], n of each.  p >= 1
 * gives unscale(min_score), p <= 0 unscale(max_score); otherwise the reference's binary search of the descending
 * table with its probe sequence (it decides which index of a run of equal values comes back).  `unscale` is the f32
 * arithmetic of dist.rs:84-88. */
int lm_hip_dists_scores(lm_hip_ctx *ctx, const lm_hip_dists *dists, const double *pvalues, float *scores);
/* ScoreDistribution::pvalue (dist.rs:91-101) of sum(counts) scores in one call: counts[i] consecutive scores belong to
 * matrix i, each `score_stride_bytes` (>= 4) behind the last -- so `&hits[0].score` with sizeof(lm_hip_set_hit) or
 * sizeof(lm_hip_hit), or a plain f32 array with a stride of 4, exactly the per-matrix layout the batch and set scans
 * return.  Writes one f64 per score.  scaled = round((score - M * offset) * scale) (dist.rs:77-81) converted as Rust's
 * `as i32` does (saturating; NaN gives 0); scaled < min_score gives 1, scaled >= sf_len gives 0, else sf[scaled]. */
int lm_hip_dists_pvalues(lm_hip_ctx *ctx, const lm_hip_dists *dists, const size_t *counts, const float *scores,
                         size_t score_stride_bytes, double *pvalues);
int lm_hip_dists_destroy(lm_hip_dists *dists);

/* Scanner (scan.rs:96-250), collected: every position with score >= threshold and
 * position + M <= L (scan.rs:185-190), as (position, f32 score) sorted by position
 * (the reference yields them in block-LIFO order and callers sort, scan.rs:291).
 * Like the reference Scanner (scan.rs:169-198) it finds candidates with a discretised
 * over-estimate of the PSSM (a packed 16-bit prefilter here, u8 DiscreteMatrix there) and
 * re-scores them exactly in f32, so the hits are those of the exact scores;
 * lm_hip_ctx_set_prefilter(ctx, 0) scores every position in f32 instead (same result).
 * Errors with LM_HIP_ERR_WRAP if wrap < M-1 (scan.rs:127-131 panics).
 * *hits is malloc'ed (NULL when *n == 0); release with lm_hip_free. */
int lm_hip_scan_f32(lm_hip_ctx *ctx, const lm_hip_pssm *pssm, const lm_hip_seq *seq,
                    float threshold, lm_hip_hit **hits, size_t *n);

/* Scanner::max EXACTLY as the reference computes it (scan.rs:200-249) -- which is not "the best
 * hit": the u8 scores of the DiscreteMatrix steer the walk.  Cells are visited in row-major
 * order (blocks ascending, Threshold order inside a block); a cell whose u8 score reaches the
 * current level is re-scored in f32 and replaces the best hit when its score is greater, or
 * equal at a greater position, and the level becomes ITS u8 score; while no hit is held the
 * first candidate is taken as it is (no `score >= threshold` test) and the level stays the
 * scaled threshold; positions are not tested against position + M <= L, and a candidate whose
 * window leaves the striped matrix makes the reference panic -- LM_HIP_ERR_BAD_ARGS here.
 *   dweights  the DiscreteMatrix's u8 weights (HOST, M x dweights_stride; pwm/mod.rs:754-791)
 *   saturate  1: the u8 adds of the SIMD back-ends (avx2.rs:336), 0: Generic's wrapping `+=`
 *   level     dm.scale(threshold), or dm.scale(best pending score) when `have`
 *   have / position / score   the best hit among those already collected and not yet yielded
 *             (scan.rs:207-210; 0 on a fresh scanner)
 *   first_row the row the scanner has reached (scan.rs `self.row`; 0 on a fresh scanner)
 * Runs on the device window by window (u8 + f32 scores of a window, an ordered parallel search
 * per update of the walk's state): ~5 ms per Gbp.  Synchronises. */
int lm_hip_scan_max_f32(lm_hip_ctx *ctx, const lm_hip_pssm *pssm, const lm_hip_seq *seq,
                        const uint8_t *dweights, size_t dweights_stride, int saturate, unsigned level,
                        int have, size_t position, float score, size_t first_row, int *found,
                        lm_hip_hit *best);

/* ---- Encode / Stripe (device pointers) ------------------------------------ */

/* Encode::encode_into (pli/mod.rs:56-66): ASCII -> symbol index.  alphabet is
 * 'D' (abc.rs:91-135) or 'P' (abc.rs:193-256).  lossy != 0 maps unknown bytes
 * to the default symbol (seq.rs:122-129) and never fails; otherwise the first
 * invalid byte's index is stored in *bad_index and LM_HIP_ERR_INVALID_SYMBOL
 * returned.  Synchronises. */
int lm_hip_encode_dptr(lm_hip_ctx *ctx, char alphabet, const uint8_t *d_ascii, size_t len,
                       int lossy, uint8_t *d_dst, size_t *bad_index);

/* Stripe::stripe_into (pli/mod.rs:178-200) + configure_wrap(wrap)
 * (seq.rs:369-381): writes ceil(len/cols)+wrap rows of `stride` bytes.
 * Bytes past `cols` in each row (struct padding of the reference's Row, unspecified there)
 * are set to the default symbol, like every element of a fresh row (dense.rs:144-147
 * `resize_with(rows, Default::default)`), so every byte of the matrix is a valid symbol. */
int lm_hip_stripe_dptr(lm_hip_ctx *ctx, const uint8_t *d_encoded, size_t len, size_t cols,
                       uint8_t default_symbol, size_t wrap, uint8_t *d_data, size_t stride);

/* StripedSequence::configure_wrap (seq.rs:369-381) on a resident matrix that
 * has room for rows + new_wrap rows. */
int lm_hip_configure_wrap_dptr(lm_hip_ctx *ctx, uint8_t *d_data, size_t rows, size_t stride,
                               size_t cols, size_t new_wrap, uint8_t default_symbol);

/* ---- resident handles ------------------------------------------------------ */

/* Upload an existing StripedSequence (seq.rs:288-294): data = matrix()[0].as_ptr(),
 * rows_total = matrix().rows() (incl. wrap -- any wrap, e.g. configure_wrap(max_m) of the
 * CLI), k = alphabet size (default symbol = k-1).  The `cols` live bytes of every row must
 * be symbols < k (LM_HIP_ERR_INVALID_SYMBOL otherwise; the reference's symbols are enums,
 * abc.rs:113-135).  The raw *_dptr entry points do NOT check this: bytes >= k there read
 * past the PSSM tables (garbage scores), which is the caller's precondition to keep.
 * Every entry point that takes a matrix (PSSM handle or discrete weights) AND a sequence
 * handle returns LM_HIP_ERR_BAD_ARGS, before anything is launched, when the matrix's
 * alphabet size differs from the handle's k (the reference's ScoringMatrix<A> and
 * StripedSequence<A> share `A`).  The raw *_dptr and host-pointer forms carry no
 * alphabet for the sequence: matching it there stays the caller's contract. */
int lm_hip_seq_upload(lm_hip_ctx *ctx, const uint8_t *data, size_t rows_total, size_t stride,
                      size_t cols, size_t wrap, size_t length, size_t k, lm_hip_seq **out);
/* The same for a matrix that already lives on the device and stays the CALLER's (a buffer of the
 * host application, a torch tensor, one row shard of a multi-GPU job): nothing is copied or
 * checked, lm_hip_seq_destroy does not free it.  rows_total rows (incl. `wrap` wrap rows) are
 * valid; the buffer has room for capacity_rows >= rows_total rows, and
 * lm_hip_seq_configure_wrap grows the wrap inside that room only (LM_HIP_ERR_CAPACITY beyond). */
int lm_hip_seq_adopt_dptr(lm_hip_ctx *ctx, uint8_t *d_data, size_t rows_total, size_t capacity_rows,
                          size_t stride, size_t cols, size_t wrap, size_t length, size_t k,
                          lm_hip_seq **out);
/* EncodedSequence::to_striped (seq.rs:168-175) on the device: uploads `len`
 * symbol bytes (each < k, else LM_HIP_ERR_INVALID_SYMBOL) and stripes them there. */
int lm_hip_seq_from_encoded(lm_hip_ctx *ctx, const uint8_t *encoded, size_t len, size_t cols,
                            size_t k, lm_hip_seq **out);
/* Same, from ASCII text: encode (strict or lossy) + stripe on the device. */
int lm_hip_seq_from_ascii(lm_hip_ctx *ctx, char alphabet, const uint8_t *ascii, size_t len,
                          size_t cols, int lossy, lm_hip_seq **out, size_t *bad_index);
/* DNA packed 4 bases per byte -- base i in bits 2*(i%4).. of byte i/4, values A0 C1 T2 G3 (the
 * Nucleotide discriminants, abc.rs:115-135): a quarter of the bytes over PCIe, unpacked straight
 * into the striped matrix (pli/mod.rs:178-200 layout).  N positions: n_runs = n_run_count pairs
 * {start, size} (the .2bit container's nBlockStarts / nBlockSizes; a genome's N are few long runs)
 * and / or n_mask, one bit per base (bit i%8 of byte i/8 set: position i is N); both may be NULL /
 * 0.  What a host that keeps genomes in 2-bit form ("ship raw/2-bit sequence") hands
 * over instead of an EncodedSequence. */
int lm_hip_seq_from_2bit(lm_hip_ctx *ctx, const uint8_t *packed, const uint8_t *n_mask,
                         const uint64_t *n_runs, size_t n_run_count, size_t len, size_t cols,
                         lm_hip_seq **out);
/* StripedSequence::configure_wrap (seq.rs:369-381); `m` = wrap rows wanted. */
int lm_hip_seq_configure_wrap(lm_hip_ctx *ctx, lm_hip_seq *seq, size_t m);
/* len(), wrap(), matrix().rows() - wrap(), stride, cols, device pointer. */
int lm_hip_seq_info(const lm_hip_seq *seq, size_t *length, size_t *wrap, size_t *rows,
                    size_t *stride, size_t *cols, const uint8_t **d_data);
/* Copies (rows+wrap) x stride bytes back. */
int lm_hip_seq_download(lm_hip_ctx *ctx, const lm_hip_seq *seq, uint8_t *dst);
int lm_hip_seq_destroy(lm_hip_seq *seq);

/* StripedScores::empty() (scores.rs:118-121). */
int lm_hip_scores_create(lm_hip_ctx *ctx, size_t cols, lm_hip_scores **out);
int lm_hip_scores_info(const lm_hip_scores *scores, size_t *rows, size_t *stride, size_t *cols,
                       size_t *max_index, const float **d_data);
/* Copies rows x stride floats back. */
int lm_hip_scores_download(lm_hip_ctx *ctx, const lm_hip_scores *scores, float *dst);
/* Rows [row_begin, row_end) only, (row_end - row_begin) x stride floats: what
 * `scores[i]` (Index<usize>, scores.rs:246-254) and windowed reads need without moving
 * a multi-gigabyte matrix. */
int lm_hip_scores_download_rows(lm_hip_ctx *ctx, const lm_hip_scores *scores, size_t row_begin,
                                size_t row_end, float *dst);
int lm_hip_scores_destroy(lm_hip_scores *scores);

/* Score::score_rows_into on handles; resizes `scores` like scores.resize. */
int lm_hip_score_rows_into(lm_hip_ctx *ctx, const lm_hip_pssm *pssm, const lm_hip_seq *seq,
                           size_t row_begin, size_t row_end, lm_hip_scores *scores);
/* Score::score_into (pli/mod.rs:109-117): rows = matrix.rows() - wrap. */
int lm_hip_score_into(lm_hip_ctx *ctx, const lm_hip_pssm *pssm, const lm_hip_seq *seq,
                      lm_hip_scores *scores);
/* Maximum::argmax / max, Threshold::threshold on a resident StripedScores. */
int lm_hip_argmax(lm_hip_ctx *ctx, const lm_hip_scores *scores, int *found,
                  lm_hip_coords *best, float *value);
int lm_hip_max(lm_hip_ctx *ctx, const lm_hip_scores *scores, int *found, float *value);
int lm_hip_threshold(lm_hip_ctx *ctx, const lm_hip_scores *scores, float t,
                     lm_hip_coords **coords, size_t *n);

/* ---- row-sharded jobs across the GPUs of a node --------------- */

/*
 * The path shards by ROW RANGES: Score::score_rows_into takes `rows: Range<usize>` for exactly
 * this (pli/mod.rs:72-78) and output row r needs input rows r .. r+M-1 only (pli/mod.rs:99-101).
 * One process per GPU holds rows [a_g, b_g) of the striped matrix plus an M-1-row halo and
 * scores them with the entry points above -- no collective.  What has to come out is what
 * StripedScores::{argmax, max, threshold} return for the WHOLE matrix (scores.rs:181-213);
 * the functions below produce it over RCCL (bound directly by this library: librccl.so.1 is
 * opened on first use; LM_HIP_ERR_COMM when it is absent).  Collectives: every rank of the
 * communicator must make the same call, with arguments that are valid on every rank or on none
 * (argument errors are reported before the collective is entered; the one per-shard condition,
 * a shard shorter than the halo, is exchanged WITH the collective and reported on every rank).
 * Waits are bounded: a collective that does not complete within LM_HIP_COMM_TIMEOUT_MS
 * (environment, read by lm_hip_comm_create; default 120000, 0 = wait for ever) -- a peer died or
 * never made the call -- aborts the communicator (ncclCommAbort) and returns LM_HIP_ERR_COMM,
 * as does every later call on it; destroy it and make a new one.  Synchronous collectives
 * (context stream) and pipelined ones (the communicator's side stream) are ordered against each
 * other on the device, so they may be mixed freely from one host thread.
 */

/* A StripedScores that is one row shard: enabled = 0 when it does NOT hold the matrix's first
 * row, so Maximum::argmax's "scores[0][0] is NaN -> (0,0)" rule (pli/mod.rs:142-146) is skipped
 * by lm_hip_argmax and by the maximum the store kernel tracks in lm_hip_score_into.  Default 1. */
int lm_hip_scores_set_first_cell_rule(lm_hip_scores *scores, int enabled);

/* The merge rule itself, on host arrays (for hosts with their own transport -- MPI, a Rust
 * channel): n per-shard results in ascending row order, rows already GLOBAL, each computed
 * with the first-cell rule on the shard holding row 0 only.  Result = Maximum::argmax of the
 * whole matrix (pli/mod.rs:135-155): greatest value; ties -> the LAST cell in (row, col)
 * order; NaN never wins except as that first-cell (0,0).  No device needed. */
int lm_hip_combine_argmax(const int *found, const lm_hip_coords *best, const float *value, size_t n,
                          int *found_out, lm_hip_coords *best_out, float *value_out);

#define LM_HIP_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank, hand the 128 bytes to the others (MPI_Bcast, a file, a
 * torch store ...), then every rank calls lm_hip_comm_create (ncclCommInitRank; blocks until
 * all nranks ranks arrive).  One GPU per rank. */
int lm_hip_comm_unique_id(uint8_t *id);
int lm_hip_comm_create(lm_hip_ctx *ctx, const uint8_t *id, int nranks, int rank, lm_hip_comm **out);
int lm_hip_comm_destroy(lm_hip_comm *comm);
int lm_hip_comm_info(const lm_hip_comm *comm, int *rank, int *nranks);

/* Set-up: fills rows [rows, rows + halo_rows) of this rank's shard with the first halo_rows rows
 * of rank+1's shard; the last rank receives rank 0's rows turned into the reference's wrap rows
 * (seq.rs:373-378: wrap[i][j] = data[i][j+1], last column = default symbol).  One all_gather
 * of halo_rows x stride bytes per rank.  Every shard needs >= halo_rows rows.  Synchronises. */
int lm_hip_exchange_halo_dptr(lm_hip_ctx *ctx, lm_hip_comm *comm, uint8_t *d_shard, size_t rows,
                              size_t stride, size_t cols, size_t halo_rows, uint8_t default_symbol);

/* StripedScores::argmax / max (scores.rs:181-192) of the whole matrix from this rank's shard
 * result (row relative to the shard; computed with first_cell_rule = (row_offset == 0)) --
 * one all_gather of a 32-byte record per rank, then lm_hip_combine_argmax.  Every rank gets
 * the same answer, rows GLOBAL. */
int lm_hip_merge_argmax(lm_hip_ctx *ctx, lm_hip_comm *comm, int found_local,
                        const lm_hip_coords *best_local, float value_local, size_t row_offset,
                        int *found, lm_hip_coords *best, float *value);
/* The same starting from the resident shard: uses the maximum the store kernel tracked when
 * lm_hip_score_into wrote `scores` (with lm_hip_scores_set_first_cell_rule(scores,
 * row_offset == 0)), else one pass over the shard; the record never leaves the device before
 * the all_gather. */
int lm_hip_argmax_sharded(lm_hip_ctx *ctx, lm_hip_comm *comm, const lm_hip_scores *scores,
                          size_t row_offset, int *found, lm_hip_coords *best, float *value);
/* The same in two halves, for a host that scores shard after shard (Scanner-style block loops,
 * scan.rs:174-178; the CLI's job loop, main.rs:502-561): _begin enqueues the shard record, its
 * all_gather and the read-back (the last two on a stream of the communicator's own) and returns at
 * once with a ticket; `scores` may be overwritten by the next lm_hip_score_into right away.  _end
 * waits for that merge only and applies lm_hip_combine_argmax.  At most two merges in flight per
 * communicator; every rank must issue the same sequence of collectives; one host thread per
 * communicator. */
int lm_hip_argmax_sharded_begin(lm_hip_ctx *ctx, lm_hip_comm *comm, const lm_hip_scores *scores,
                                size_t row_offset, int *ticket);
int lm_hip_argmax_sharded_end(lm_hip_ctx *ctx, lm_hip_comm *comm, int ticket, int *found,
                              lm_hip_coords *best, float *value);
/* Maximum::max (pli/mod.rs:158-160) when no NaN can occur (NaN contributions are dropped). */
int lm_hip_merge_max(lm_hip_ctx *ctx, lm_hip_comm *comm, int found_local, float value_local,
                     int *found, float *value);
/* StripedScores::threshold (scores.rs:207-213) of the whole matrix: this rank's row-major list
 * (rows relative to the shard) -> the concatenation over ranks in rank order with GLOBAL rows,
 * which is the reference's row-major push order (pli/mod.rs:212-218).  Counts travel by
 * all_gather, lists by one exact-length broadcast per rank.  *all is malloc'ed on every rank
 * (NULL when *n_all == 0); release with lm_hip_free. */
int lm_hip_merge_threshold(lm_hip_ctx *ctx, lm_hip_comm *comm, const lm_hip_coords *coords, size_t n,
                           size_t row_offset, lm_hip_coords **all, size_t *n_all);

/* ---- host-pointer convenience forms (synchronous, PCIe both ways) ---------- */

/* Exactly what a Rust shim can obtain from &StripedSequence / &DenseMatrix / &mut StripedScores: pageable host
 * matrices in, pageable host matrices out (csrc/hostptr.hip; lanes: host_lane.hip, large calls: host_pipe.hip).  No context argument: every calling host thread is given
 * a lane of its own (context + stream, persistent staging, a cache of device PSSM tables keyed on the weights), so
 * threads overlap.  Lanes sit on ONE device unless told otherwise: $LM_HIP_DEVICE (read once per process; must name a
 * usable ordinal), else the HIP device current in the thread that made the first host-pointer call -- so a job of one
 * process per GPU never opens contexts on its neighbours' devices.  lm_hip_host_spread_lanes(1) deals new lanes
 * round-robin over every usable device instead: the reference's parallel axis is the CLI's worker threads over
 * (motif, sequence) jobs (lightmotif-cli main.rs:240-378), which then spread over the GPUs and PCIe links of a node with
 * one call added to the host; lm_hip_host_bind_thread places one thread.  Large calls (>= 96 MB of scores) run as a tile pipeline over a per-device ring of
 * pinned buffers (allocated on, and served by helper threads bound to, the GPU's NUMA node) and take turns on it.
 * 1 B per position travels up and 4 B down per lm_hip_score_f32 call. */
int lm_hip_score_f32(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols,
                     size_t wrap, size_t length,
                     const float *pssm, size_t m, size_t pssm_stride, size_t k,
                     size_t row_begin, size_t row_end,
                     float *out, size_t out_stride, size_t *out_rows, size_t *max_index);
/* Score<u8, A, C>::score_rows_into with a DiscreteMatrix's weights on host matrices (pwm/mod.rs:754-791; the AVX2 impl is
 * pli/mod.rs:437-476 over avx2.rs:294-347) -- what Scanner::next calls per block (scan.rs:174-178).  `saturate` != 0: the
 * SIMD back-ends' saturating adds (avx2.rs:336), 0: Generic's wrapping `+=`.  Same conventions as lm_hip_score_f32. */
int lm_hip_score_u8_host(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols,
                         size_t wrap, size_t length,
                         const uint8_t *weights, size_t m, size_t weights_stride, size_t k,
                         size_t row_begin, size_t row_end, int saturate,
                         uint8_t *out, size_t out_stride, size_t *out_rows, size_t *max_index);
int lm_hip_argmax_f32(const float *scores, size_t rows, size_t stride, size_t cols,
                      int *found, lm_hip_coords *best, float *value);
/* Maximum::max on a host matrix (pli/mod.rs:158-160; SURVEY 8b export list). */
int lm_hip_max_f32(const float *scores, size_t rows, size_t stride, size_t cols,
                   int *found, float *value);
int lm_hip_threshold_f32(const float *scores, size_t rows, size_t stride, size_t cols, float t,
                         lm_hip_coords **coords, size_t *n);
/* Scanner (scan.rs:96-250) on a HOST StripedSequence: what `Dispatch::Hip` specialises `Scanner` onto instead of driving
 * its 256-row block loop through the Score<u8> arm (a block is ~19 us of launch + link latency for 8 192 cells).  The striped
 * matrix goes up once (1 B per position), then lm_hip_scan_f32 / lm_hip_scan_max_f32 run on it; same results, same
 * conventions, same errors as those.  A host that scans one sequence with MANY motifs should upload it once
 * (lm_hip_seq_upload) and use the resident forms. */
int lm_hip_scan_f32_host(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols,
                         size_t wrap, size_t length,
                         const float *pssm, size_t m, size_t pssm_stride, size_t k,
                         float threshold, lm_hip_hit **hits, size_t *n);
int lm_hip_scan_max_f32_host(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols,
                             size_t wrap, size_t length,
                             const float *pssm, size_t m, size_t pssm_stride, size_t k,
                             const uint8_t *dweights, size_t dweights_stride, int saturate, unsigned level,
                             int have, size_t position, float score, size_t first_row,
                             int *found, lm_hip_hit *best);

/* ---- the `Dispatch::Hip` policy --------------------------------------------------------------------
 *
 * lightmotif/src/pli/dispatch.rs has seven `match self.backend` sites, and `Scanner` hard-codes `Pipeline<A, Dispatch>`
 * (scan.rs:166).  A `Hip` variant must say what it does at EACH of them: a call on host matrices pays a launch, a
 * synchronisation and the link both ways, so below some size -- and for operations that only move bytes -- the right arm is
 * the CPU tier the variant carries (`Hip { cpu: Avx2 | Sse2 | Neon | Generic }` = what Pipeline::dispatch() would have
 * picked without a GPU, pli/mod.rs:269-308), never `_ => Generic`.  lm_hip_host_crossover returns, per site, the number of
 * cells (rows x columns of the call) from which the host-pointer entry point is expected to beat ONE thread of the AVX2
 * tier: SIZE_MAX = the site stays on the CPU tier at every size (Encode, Stripe: one pass over bytes that a core streams
 * faster than the link carries them; Maximum / Threshold on u8: Scanner-internal, specialised away), 0 = always the GPU.
 * The constants are measured (tools/crossover.py on MI355X + EPYC 9575F, profiles/r05_crossover.json) and a function of
 * the motif length where the CPU's cost is (Score: CPU time ~ M x cells, GPU time ~ latency + 5 B x cells / link). */
typedef enum lm_hip_host_op {
    LM_HIP_OP_ENCODE = 0,        /* Encode::encode_into           dispatch.rs:58-77   -> CPU tier            */
    LM_HIP_OP_SCORE_F32 = 1,     /* Score<f32>::score_rows_into   dispatch.rs:79-108  -> lm_hip_score_f32     */
    LM_HIP_OP_SCORE_U8 = 2,      /* Score<u8>::score_rows_into    dispatch.rs:110-137 -> lm_hip_score_u8_host */
    LM_HIP_OP_STRIPE = 3,        /* Stripe::stripe_into           dispatch.rs:139-153 -> CPU tier            */
    LM_HIP_OP_MAXIMUM_F32 = 4,   /* Maximum<f32>::argmax / max    dispatch.rs:155-179 -> lm_hip_argmax_f32 / lm_hip_max_f32 */
    LM_HIP_OP_MAXIMUM_U8 = 5,    /* Maximum<u8>::argmax / max     dispatch.rs:181-205 -> CPU tier            */
    LM_HIP_OP_THRESHOLD_F32 = 6, /* Threshold<f32>::threshold     dispatch.rs:205     -> lm_hip_threshold_f32 */
    LM_HIP_OP_THRESHOLD_U8 = 7,  /* Threshold<u8>::threshold      dispatch.rs:207     -> CPU tier            */
    LM_HIP_OP_SCAN = 8           /* Scanner::next / max           scan.rs:166-249     -> lm_hip_scan_f32_host / lm_hip_scan_max_f32_host */
} lm_hip_host_op;
/* m = motif length (0 where it plays no part), k = alphabet size.  LM_HIP_ERR_BAD_ARGS for an unknown op. */
int lm_hip_host_crossover(int op, size_t m, size_t k, size_t *cells);
/* The reference picks its back-end per HOST, at run time (pli/mod.rs:269-308); so does the policy.  The model behind
 * lm_hip_host_crossover is  GPU call ~ t0 + g x cells,  CPU tier ~ (c + c_row x M) x cells,  crossover = t0 / (c + c_row M - g)
 * (never while the tier costs less than 1.25 x the link per cell).  The compiled constants are one box's (EPYC 9575F, PCIe
 * Gen5); these calls replace them with this process's own:
 *   lm_hip_host_calibrate   measures the GPU side (t0, g) of every site that can leave the tier by timing the host-pointer
 *                           entry points themselves on synthetic matrices (8 192 and 4 Mi cells), within ~budget_ms in total
 *                           (a few tens of milliseconds suffice).  Once per process unless `force`; thread-safe.
 *   lm_hip_host_set_cpu_cost  the CPU tier's side, which only the caller can time (its tier is Rust code the library never
 *                           sees): ns per cell, and ns per cell and motif row (0 where M plays no part).
 *   lm_hip_host_set_crossover pins the answer for a site whatever M (SIZE_MAX = never the GPU, 0 = always); (size_t)-2
 *                           (LM_HIP_CROSSOVER_MODEL) unpins it.
 *   lm_hip_host_cost_model  reads the constants in force and whether the GPU side was measured here.  Pointers may be NULL. */
#define LM_HIP_CROSSOVER_MODEL ((size_t)-2)
int lm_hip_host_calibrate(double budget_ms, int force);
int lm_hip_host_set_cpu_cost(int op, double ns_per_cell, double ns_per_cell_and_motif_row);
int lm_hip_host_set_crossover(int op, size_t cells);
int lm_hip_host_cost_model(int op, double *t0_us, double *gpu_ns_per_cell, double *cpu_ns_per_cell, double *cpu_ns_per_cell_and_motif_row,
                           int *gpu_side_measured);

/* Hands back what the host-pointer functions keep between calls: the pinned rings of the tile pipelines (128 MB of
 * page-locked memory per device used), their device tiles, and the device staging AND reduction scratch of this thread's
 * lane and of lanes whose threads have exited; lanes of other live threads hand theirs back at the end of their next
 * call.  Contexts and cached PSSM tables stay; the next call sets up again what it needs.  Safe at any time (waits for
 * a large call in flight); for hosts that score a genome and then sit idle. */
int lm_hip_host_trim(void);
/* != 0: NEW host-pointer lanes are dealt round-robin over every usable device (one process driving a whole node); 0 (the
 * default): every lane on the process's one host-pointer device (see above).  Lanes that exist stay where they are. */
int lm_hip_host_spread_lanes(int enabled);
/* != 0: a lane keeps the device copy of the score matrix its last lm_hip_score_f32 produced, and lm_hip_argmax_f32 /
 * lm_hip_max_f32 / lm_hip_threshold_f32 called by the same thread on that very matrix (same pointer, shape and stride) reduce
 * the copy instead of uploading the matrix again -- the reference's own benchmark shape, `score_into` followed by `argmax`
 * (lightmotif-bench/dna.rs:81-116: 150 -> ~110 us per iteration at 464 kbp).  The caller promises not to write to the matrix
 * between the two calls; the library checks a 64-bit digest of 67 sampled cells and falls back to the upload when it differs,
 * which catches a recycled buffer, not a deliberate single-cell edit.  0 (the default): every call uploads what it is given.
 * Process-wide; always LM_HIP_OK. */
int lm_hip_host_reuse_scores(int enabled);
/* How many calls of the calling thread's lane took the kept copy so far (a diagnostic for tests and tools). */
int lm_hip_host_reuse_count(size_t *count);
/* Puts the calling thread's host-pointer lane on `device` (a HIP ordinal from lm_hip_device_ordinal) from its next call
 * on; -1 = back to the automatic placement ($LM_HIP_DEVICE, else the process's device or the round-robin).  For hosts that place their worker
 * threads themselves (one thread per GPU, threads pinned next to their GPU). */
int lm_hip_host_bind_thread(int device);
/* Where the calling thread's lane is (creates it if need be): its device ordinal, the NUMA node the platform reports for
 * that GPU (-1: none reported) and how many CPUs of that node the pipeline's helper threads are confined to (0: unbound).
 * Any pointer may be NULL (not all three). */
int lm_hip_host_lane_info(int *device, int *numa_node, int *helper_cpus);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTMOTIF_HIP_H */
