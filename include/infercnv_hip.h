/*
 * infercnv_hip.h -- C ABI of the MI355X (gfx950) CNV-inference engine.
 *
 * This is the drop-in boundary for ONE hot path of icbi-lab/infercnvpy:
 * the per-chunk numeric kernel `_infercnv_chunk` (reference
 * src/infercnvpy/tl/_infercnv.py:411-457) together with the pieces of the
 * `infercnv` driver that touch every matrix element (reference mean,
 * :359-408; chunk fan-out/vstack, :120-139) and the `cnv_score` reduction
 * (src/infercnvpy/tl/_scores.py:65-68).
 *
 * The reference has no FFI; its seam is a Python function called once per
 * 5000-cell chunk from a ProcessPoolExecutor worker.  A maintainer binds this
 * library with ctypes and calls it from `infercnv()` in
 * place of `process_map(_infercnv_chunk, ...)`.
 *
 * Conventions
 *   - plain C types only; every data pointer is a DEVICE pointer (HBM) unless
 *     the parameter name starts with `h_` (host);
 *   - every function returns an icv_status (0 = ok); `icv_last_error()` returns
 *     a thread-local message for the last failure; no C++ exception crosses;
 *   - the caller owns all buffers; the only library-owned object is the opaque
 *     plan (create / destroy);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls
 *     are asynchronous on that stream unless stated otherwise.
 */
#ifndef INFERCNV_HIP_H
#define INFERCNV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ICV_OK = 0,
    ICV_ERR_INVALID = 1,     /* bad argument (maps to Python ValueError)            */
    ICV_ERR_UNSUPPORTED = 2, /* configuration exceeds an implementation limit       */
    ICV_ERR_HIP = 3,         /* HIP runtime failure (message has the hipError name) */
    ICV_ERR_NOMEM = 4
} icv_status;

enum { ICV_F32 = 0, ICV_F64 = 1 };
enum { ICV_DENSE = 0, ICV_CSR = 1 };

/* flags for icv_infercnv_* */
enum {
    ICV_FLAG_TRUNC_TO_INT = 1, /* bounded centring of an integer matrix keeps the matrix dtype
                                  (reference :428): centred values are truncated toward zero */
    ICV_FLAG_ROUND_F32 = 2,    /* bounded centring of a float32 matrix against a float64 reference:
                                  differences are rounded to float32 (same line)              */
    ICV_FLAG_NO_APPLY = 4      /* icv_infercnv_run: compute the thresholds, leave `out` un-thresholded */
};

/* A cells x genes expression matrix resident in HBM. */
typedef struct {
    int32_t format;         /* ICV_DENSE | ICV_CSR                                     */
    int32_t dtype;          /* ICV_F32 | ICV_F64 (dtype of `values`)                   */
    int64_t n_rows;         /* cells                                                   */
    int32_t n_cols;         /* genes = n_cols_all of the plan                          */
    int32_t _pad;           /* dense: column offset of `values` inside its row when the matrix is a column view of a
                               wider one (0 otherwise); only icv_colchain looks at it (which loads stay in bounds).
                               csr: optional hint, the number of stored entries MOST rows stay under (e.g. the 99.9 %
                               quantile of the row lengths; 0 = unknown): the stored-entries kernel sizes its per-cell
                               entry slots with it -- a performance hint only, any value gives the same results      */
    int64_t ld;             /* dense: row stride in elements (>= _pad + n_cols)        */
    const void *values;     /* dense: n_rows x ld row-major; csr: nnz values           */
    const int64_t *indptr;  /* csr: n_rows + 1                                         */
    const int32_t *indices; /* csr: nnz column indices, unique and ascending within a row */
    int64_t csr_begin;      /* csr: host copies of indptr[0] and indptr[n_rows]; both 0 = unknown  */
    int64_t csr_end;        /*      (the prepared-entry fast path needs them to size its workspace) */
} icv_matrix;

typedef struct icv_plan_s *icv_plan_t;

typedef struct {
    int32_t n_cols_all;   /* columns of the input matrix                               */
    int32_t n_genes_used; /* columns that fall in a window-bearing chromosome          */
    int32_t n_chr;
    int32_t window;
    int32_t step;
    int32_t n_windows;    /* W = sum_c W_c  (reference :218, :227-236)                  */
    int32_t block;        /* B: genes per partial-sum block (1 = direct form)          */
    int32_t n_blocks;     /* padded blocks over all chromosomes                        */
    int32_t padded_len;   /* LDS row length in elements                                */
    int32_t lds_bytes_f32;/* dynamic LDS per workgroup for float32 input               */
    int32_t lds_bytes_f64;
    int32_t workgroups_per_cu_f32;
} icv_plan_info;

/* ---- planning (host only, no GPU needed) -------------------------------------------------
 * Gene/position indexing contract (reference :327, :350-351): the caller sorts the genes of
 * every window-bearing chromosome by `start` and concatenates chromosomes in natural order.
 *   h_col_pos[g]      position of input column g in that concatenation, or -1 if the column is
 *                     masked (no position / excluded chromosome / chrM / non-"chr" contig)
 *   h_chrom_offsets   n_chr + 1 offsets into the concatenation
 * The library derives the window table: per chromosome with G_c genes,
 *   window < G_c : W_c = ceil((G_c - window + 1) / step) pyramid windows  (:205-218)
 *   otherwise    : one flat window over all G_c genes                     (:227-236)
 * Concurrency: the tables of a plan are immutable after creation, but the plan also owns the per-call device
 * workspace of the compute entry points (moment partials, hand-back lists, CSR staging): ONE compute call at a
 * time per plan.  A second call entering while one is in its launch sequence fails with ICV_ERR_INVALID ("plan
 * busy") instead of racing.  Successive calls on one plan are ordered on the device: a call enqueued on another
 * stream than the plan's previous call first waits (hipStreamWaitEvent) for that call's kernels, so the shared
 * workspace is never used by two calls at once; calls on different plans are independent.
 */
int icv_plan_create(int32_t n_cols_all, const int32_t *h_col_pos, int32_t n_chr,
                    const int32_t *h_chrom_offsets, int32_t window, int32_t step, icv_plan_t *out);
void icv_plan_destroy(icv_plan_t plan);
int icv_plan_get_info(icv_plan_t plan, icv_plan_info *h_info);
/* first window index of every chromosome = the values of uns["cnv"]["chr_pos"] (:335-337) */
int icv_plan_chr_pos(icv_plan_t plan, int32_t *h_chr_pos /* n_chr */);
/* window table in sorted-gene coordinates: window j covers [start, start+len) */
int icv_plan_window_table(icv_plan_t plan, int32_t *h_start /* W */, int32_t *h_len /* W */);
/* Which smoothing kernel the plan's last compute call (icv_infercnv_smooth / _run / icv_gene_values) launched:
 * diagnostics and tests ("this input really took the CSR stored-entries kernel"). */
enum {
    ICV_KERNEL_NONE = 0,
    ICV_KERNEL_GENERIC = 1, /* k_smooth: any dtype / format / geometry that fits LDS                      */
    ICV_KERNEL_WS = 2,      /* k_smooth_ws: dense float32, block form                                     */
    ICV_KERNEL_WS_CSR = 3,  /* k_csr_prepare + k_smooth_ws: CSR float32, row rebuilt in LDS               */
    ICV_KERNEL_X16 = 4,     /* k_smooth_x16: dense float32, window 100 or 250 / step 10                   */
    ICV_KERNEL_SD = 5,      /* k_smooth_sd: CSR float32, block form, stored entries only (prefix sums)    */
    ICV_KERNEL_SPLIT = 6,   /* chromosome groups (row larger than LDS) + median on float64 windows in HBM */
    ICV_KERNEL_X16_FINITE = 7 /* k_smooth_x16<FINITE>: the same kernel without NaN handling (icv_infercnv_run_finite) */
};
/* A call that passed `finite_words` launched k_smooth_x16 in both forms and the device chose between them:
 * icv_plan_last_kernel then reads the form that applied back from the device (it waits for that call) and reports
 * ICV_KERNEL_X16_FINITE or ICV_KERNEL_X16.  icv_plan_last_route never waits: the route the host picked, ICV_KERNEL_X16
 * for either form. */
int icv_plan_last_kernel(icv_plan_t plan, int32_t *h_kind);
int icv_plan_last_route(icv_plan_t plan, int32_t *h_kind);
/* How many cells the last smoothing launch on this plan handed back to k_smooth (more than 64 windows in the bins of
 * the two middle ranks; k_smooth_se: also cells with a stored NaN): the device-side counter of that launch, copied to
 * the host.  0 where the last launch was of a kernel that hands nothing back (ICV_KERNEL_GENERIC, _SPLIT) or nothing
 * was launched.  The caller has synchronised the stream of that call.  Diagnostics and tests. */
int icv_plan_last_handed_back(icv_plan_t plan, int64_t *h_n);
/* Host tables of the CSR stored-entries kernel (k_smooth_se), for tests that restate its arithmetic on the CPU:
 * *h_applies = 1 if the plan's geometry admits the kernel (else nothing more is written); per input column the
 * block of its gene (-1: masked) and the gene's offset inside the block; per block the offset of its first gene
 * inside its chromosome; per window the two packed words that name the LDS slots of its three prefix sums and the
 * wavefront totals to add (csrc/icv_plan.hpp: se_window_words).  Any of the array pointers may be NULL. */
int icv_plan_se_tables(icv_plan_t plan, int32_t *h_applies, int32_t *h_col_block /* n_cols_all */,
                       int32_t *h_col_offset /* n_cols_all */, int32_t *h_block_gene0 /* n_blocks */,
                       uint32_t *h_w0 /* W */, uint32_t *h_w1 /* W */);
/* Host tables of calculate_gene_values (reference tl/_infercnv.py:247-298: a gene's value is the mean of the kept windows
 * that contain it), for tests that check them on the CPU against the oracle: the covered genes in chromosome / position
 * order fall into RUNS that share their windows; run r averages the windows [first, first + count) (global window
 * indices) and holds `genes` genes; h_col_run[c] = the run of input column c, -1 where the gene has no value (masked
 * chromosome, or no kept window contains it: NaN in the layer, :147).  *h_n_runs is always written; the arrays (each may
 * be NULL) hold *h_n_runs / n_cols_all entries: call once with NULL arrays for the size. */
int icv_plan_gene_runs(icv_plan_t plan, int32_t *h_n_runs, int32_t *h_run_first, int32_t *h_run_count,
                       int32_t *h_run_genes, int32_t *h_col_run /* n_cols_all */);

/* ---- reference profile (reference :385, :400) --------------------------------------------
 * Per-group column sums in float64.  h/d: `row_group` (device, n_rows int32; -1 = row not in
 * any group; NULL = every row in group 0).  `sums` (device, n_groups x n_cols float64) is
 * ACCUMULATED into, so shards / ranks can add up before the caller divides by the counts.
 * Dense and CSR sums are deterministic (fixed reduction order; CSR: a 1024-thread workgroup per row slab adds ONE
 * row at a time into float64 LDS accumulators, a barrier between rows, so every column receives its addends in
 * row order; the slabs are then added in slab order).
 */
int icv_colsum(const icv_matrix *m, const int32_t *row_group, int32_t n_groups, double *sums,
               void *stream);

/* The same profile in the REFERENCE'S OWN EVALUATION ORDER, so that `reference=None` / `reference_cat` reproduce the
 * reference bit for bit (float32 sums are not associative):
 *   - np.mean(X, axis=0) of a C-contiguous matrix (reference :385, :400) is, per column, the sequential chain
 *     acc = fl(acc + x[r][g]) over the rows in order, in the matrix dtype (float32 stays float32), then acc / n;
 *   - scipy's CSR mean is the same chain over fl(x * fl(1/n)) (no division afterwards);
 *   - scipy's CSC mean is np.add.reduceat per column: first stored entry + numpy's pairwise sum of the others;
 *   - np.mean(X, axis=0) of a dense matrix stored column-major: pairwise per column (icv_colsum_pairwise below).
 * icv_colchain continues the chains: `acc` (device, n_cols values of the MATRIX dtype; zero before the first call) is
 * read, the rows `rows[0..n_sel)` of `m` (device int32, ascending; NULL = all rows of m) are added in order, and the
 * new accumulators are written back -- row pieces, slabs and shards are chained by calling in row order with the same
 * `acc`.  `scale` is used for CSR input only (1 / n of the whole group, rounded to the matrix dtype inside).
 * Columns are the only parallelism an exact chain has: one workgroup per 128..512-byte tile of a row streams its rows
 * through an LDS ring (LDS-DMA) while one wavefront adds them in order.  CSR needs 4 * (tiles + 1) bytes of temporary
 * device memory per row (stream-ordered).  Nothing is read back: the call never synchronises.
 * icv_colchain_mean: mean[c] = acc[c] / count in the dtype (dense); for CSR the accumulators already are the means.
 * icv_colmean_csc: means of a CSC matrix (colptr n_cols + 1 int64, row_idx int32, values), entries of rows with
 * row_group[row] == group only (row_group NULL: all), scale = 1 / n as above; `mean` n_cols values of the dtype. */
int icv_colchain(const icv_matrix *m, const int32_t *rows, int64_t n_sel, double scale, void *acc, void *stream);
/* The all-cell sums of a dense matrix stored COLUMN-major (numpy puts the axis with the smaller stride innermost:
 * np.mean(X, axis=0) of an F-ordered array reduces every column with its contiguous inner loop = pairwise summation,
 * over pieces of 8 192 elements, the iterator's buffer): `xt` holds n_cols columns of n_rows contiguous values each,
 * `ld` elements apart (the caller uploads column blocks as they lie in host memory); sums[c] = that reduction, in the
 * dtype (icv_colchain_mean divides). */
int icv_colsum_pairwise(const void *xt, int32_t dtype, int64_t n_rows, int32_t n_cols, int64_t ld, void *sums,
                        void *stream);
int icv_colchain_mean(const void *acc, int32_t dtype, int32_t n_cols, int64_t count, void *mean, void *stream);
/* icv_colchain_mean that also says whether every mean it wrote is finite: `finite_words` (device, ICV_FINITE_WORDS
 * uint32, 16-byte aligned, no need to clear them) receives one word per workgroup, non-zero where a mean is NaN or
 * infinite.  A chain that met a NaN stays NaN, one that met an infinity stays infinite or turns NaN: where `acc` holds
 * the chains over ALL rows of a matrix, all-zero words certify that every element of that matrix is finite
 * (icv_infercnv_run_finite). */
#define ICV_FINITE_WORDS 16
int icv_colchain_mean_finite(const void *acc, int32_t dtype, int32_t n_cols, int64_t count, void *mean,
                             uint32_t *finite_words, void *stream);
int icv_colmean_csc(const void *values, int32_t dtype, const int64_t *colptr, const int32_t *row_idx, int32_t n_cols,
                    const int32_t *row_group, int32_t group, double scale, void *mean, void *stream);

/* ---- the hot path ------------------------------------------------------------------------
 * Steps 1-4 of `_infercnv_chunk` (:422-442) for every row of `m`, fused in one kernel:
 *   centre on the reference (ref_hi == NULL: x - ref_lo; else bounded difference),
 *   clip to +-lfc_clip in the matrix dtype, pyramid/flat windowed mean per chromosome in
 *   float64, subtract the per-cell median over all W windows.
 * Outputs (device):
 *   out         n_rows x ldo float32, un-thresholded x_res (rows on 16-byte boundaries -- ldo % 4 == 0 and a
 *               16-byte aligned base -- let the dense fast kernel store 16 bytes per lane)
 *   cell_median n_rows float64
 *   cell_stats  n_rows x 2 float64: sum(x_res), sum(x_res^2) of the row (for the chunk std)
 * `ref_lo`/`ref_hi`: n_cols values of the matrix dtype, in input column order.
 */
int icv_infercnv_smooth(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                        double lfc_clip, int32_t flags, float *out, int64_t ldo, double *cell_median,
                        double *cell_stats, void *stream);

/* Step 5a (:450): thr[k] = dynamic_threshold * population-std over chunk k, where chunk k is rows
 * [k*chunksize - row_phase, ...) of this shard (row_phase = global index of the shard's first row
 * modulo chunksize; 0 when shards are chunk-aligned).  `thr` device float64[n_chunks]. */
int icv_chunk_thresholds(const double *cell_stats, int64_t n_rows, int64_t chunksize, int64_t row_phase,
                         int32_t n_windows, double dynamic_threshold, double *thr, void *stream);

/* Step 5b (:451): out[|x| < thr[chunk(row)]] = 0, decided in float64: an entry whose float32
 * value ties with float32(thr) is recomputed from the input in float64 before deciding. */
int icv_apply_threshold(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                        double lfc_clip, int32_t flags, float *out, int64_t ldo,
                        const double *cell_median, const double *thr, int64_t chunksize,
                        int64_t row_phase, void *stream);

/* Timings of the last icv_infercnv_run with profiling enabled (milliseconds, HIP events
 * recorded on `stream`). */
typedef struct {
    float smooth_ms;
    float thresholds_ms;
    float apply_ms;
    float total_ms;
} icv_profile;

/* Convenience: smooth -> chunk thresholds -> apply, on one stream.  `dynamic_threshold` NaN
 * disables step 5 (reference: None).  `thr` may be NULL only when step 5 is disabled.
 * `cell_stats` may be NULL: the per-cell moments are then not returned, and where the dense fast kernel runs
 * they are not formed at all (the kernel accumulates the noise-threshold moments per chunk).
 * flags | ICV_FLAG_NO_APPLY: compute `thr` but leave `out` un-thresholded (for icv_threshold_mask).
 * One call at a time per plan: the plan owns the per-call workspace (see icv_plan_create).
 * If `h_profile` is non-NULL the call records HIP events around each stage, synchronises the
 * stream before returning and fills the struct. */
int icv_infercnv_run(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                     double lfc_clip, double dynamic_threshold, int64_t chunksize, int64_t row_phase,
                     int32_t flags, float *out, int64_t ldo, double *cell_median, double *cell_stats,
                     double *thr, icv_profile *h_profile, void *stream);

/* Deferred timing for back-to-back runs: after icv_profile_begin every icv_infercnv_run on this plan (called
 * with h_profile == NULL) records HIP events around its stages on its stream WITHOUT synchronising;
 * icv_profile_collect waits for the recorded runs, fills up to max_records structs in call order, returns the
 * count and ends the deferred mode.  (bench.py: kernel time measured over the timed region with no host
 * synchronisation between steps.) */
int icv_profile_begin(icv_plan_t plan);
int icv_profile_collect(icv_plan_t plan, icv_profile *out, int32_t max_records, int32_t *n_records);

/* ---- the reference-order float32 chain by BLOCKS of rows (csrc/icv_kernel_blocks.hpp) ---------------------------
 * icv_colchain evaluates np.mean's sequential float32 chain (reference :385) at HBM stream rate on ONE GPU, but row
 * shards on several GPUs must take turns.  Inside one binade the chain is integer arithmetic (fl(s + x) = s + q ulp(s)
 * with q = round(x / ulp(s)) independent of s except at exact ties), so a block of 64 rows whose chain stays inside its
 * binade and holds no tie is ONE integer: the ranks compute them CONCURRENTLY from a float64 estimate of their start,
 * and only a scan over the records (plus the rare replays) runs in row order.  Dense float32 matrices, all rows;
 * everything else: ICV_ERR_UNSUPPORTED (use icv_colchain).  Bit-equal to icv_colchain for any estimate.
 *   workspace: device buffer of icv_colchain_blocks_workspace(n_rows, n_cols) bytes, the same for the three calls
 *   1. icv_colchain_blocks_sums:    float64 column totals of the matrix -> total[n_cols] (device); all-gather them
 *   2. icv_colchain_blocks_records: est_start[n_cols] (device float64, NULL = 0) = the estimate of the chain value
 *                                   before row 0 (sum of the earlier ranks' totals) -> the block records
 *   3. icv_colchain_blocks_scan:    acc[n_cols] (device float32, in / out) = the EXACT chain values before row 0 (from
 *                                   the previous rank) -> after the last row; columns [col0, col1) only (ranks pipeline
 *                                   over column groups); d_replayed (device, optional) += blocks replayed row by row. */
int icv_colchain_blocks_workspace(int64_t n_rows, int32_t n_cols, int64_t *bytes);
int icv_colchain_blocks_sums(const icv_matrix *m, void *workspace, double *total, void *stream);
int icv_colchain_blocks_records(const icv_matrix *m, void *workspace, const double *est_start, void *stream);
int icv_colchain_blocks_scan(const icv_matrix *m, void *workspace, float *acc, int32_t col0, int32_t col1,
                             uint64_t *d_replayed, void *stream);

/* ---- calculate_gene_values=True (reference :247-298, :443-453) -------------------------------
 * Per-gene CNV values: mean of the kept windows that contain the gene (:274-288), minus the per-cell median
 * over the covered genes (:443-444), zeroed below the chunk's noise threshold (:452-453; `thr` from
 * icv_chunk_thresholds / icv_infercnv_run; NULL = no thresholding).  `gene_out` (device, float64,
 * n_rows x ldg, ldg >= n_cols) is written completely: NaN for genes no kept window covers and for
 * masked genes (reference: reindex with NaN fill, :147).
 *
 * The windows a gene averages are the float64 windows of step 3 BEFORE the per-cell centring -- what the
 * smoothing kernel holds anyway.  icv_infercnv_run_windows is icv_infercnv_run that also writes them
 * (`win_out`: device float64, n_rows x ldw, ldw >= n_windows; NULL = plain icv_infercnv_run): the same kernel
 * as the plain call (k_smooth_x16 / k_smooth_se store them beside x_res; other geometries: the generic kernel),
 * 8 * n_windows more bytes per cell.  icv_gene_values_from_windows turns them into the gene layer in ONE kernel:
 * windows -> LDS, one value per run of genes that share their windows, weighted median by radix select, the
 * row written once in input-column order.  So `calculate_gene_values=True` costs the plain call + the windows +
 * one pass that writes 8 * n_cols bytes per cell -- no second smoothing (reference: _infercnv_chunk returns both
 * from one pass too, :438-457).
 *
 * icv_gene_values (kept): smoothing + gene layer in one call for callers that do not need X_cnv;
 * stream-ordered temporaries of 12 * n_windows bytes per row. */
int icv_infercnv_run_windows(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                             double lfc_clip, double dynamic_threshold, int64_t chunksize, int64_t row_phase,
                             int32_t flags, float *out, int64_t ldo, double *cell_median, double *cell_stats,
                             double *thr, icv_profile *h_profile, double *win_out, int64_t ldw, void *stream);
/* icv_infercnv_run_windows for a caller that formed `ref_lo` with icv_colchain_mean_finite over ALL rows `m` holds
 * (or is a part of): `finite_words` are that call's words (NULL: icv_infercnv_run_windows).  Where the input takes
 * k_smooth_x16, the kernel is launched twice back to back -- without its per-gene NaN handling, and as it is -- and
 * each launch reads the words first: all zero, the first one runs and the second returns at once, else the other way
 * round.  No host synchronisation; results are those of icv_infercnv_run_windows bit for bit.  Every other route
 * ignores the words.  Words from means over a SUBSET of the rows, or a profile from elsewhere, prove nothing: pass
 * NULL. */
int icv_infercnv_run_finite(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                            double lfc_clip, double dynamic_threshold, int64_t chunksize, int64_t row_phase,
                            int32_t flags, float *out, int64_t ldo, double *cell_median, double *cell_stats,
                            double *thr, icv_profile *h_profile, double *win_out, int64_t ldw,
                            const uint32_t *finite_words, void *stream);
int icv_gene_values_from_windows(icv_plan_t plan, const double *win, int64_t ldw, int64_t n_rows,
                                 const double *thr, int64_t chunksize, int64_t row_phase, double *gene_out,
                                 int64_t ldg, void *stream);
int icv_gene_values(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                    double lfc_clip, int32_t flags, const double *thr, int64_t chunksize,
                    int64_t row_phase, double *gene_out, int64_t ldg, void *stream);

/* ---- CSR packing of X_cnv (reference :455 `csr_matrix(x_res)`, :137 vstack) ------------------ */

/* Geometry of the streamed pack kernels for rows of n_windows float32 (host logic, no GPU needed): whether
 * icv_threshold_mask / icv_csr_fill_masked take the LDS-ring kernels at this width (given aligned rows), how the 160 KB
 * of LDS of a CU are split, and how many LDS-DMA loads a loader wavefront keeps in flight (the hardware counter holds 63). */
typedef struct {
    int32_t rows_per_round;        /* adjacent rows a workgroup takes per barrier */
    int32_t mask_streamed;         /* 1: k_thr_mask_ring applies */
    int32_t mask_ring_slots;       /* ring slots of rows_per_round rows (one being read, the others in flight) */
    int32_t mask_lds_bytes;        /* ring + the two staging blocks of mask words and counts */
    int32_t mask_loads_in_flight;  /* per loader wavefront */
    int32_t fill_streamed;         /* 1: k_csr_fill_ring applies */
    int32_t fill_ring_slots;
    int32_t fill_lds_bytes;        /* ring (rows + the round's mask rows and row offsets) + two staging blocks */
    int32_t fill_loads_in_flight;  /* loader 0 (it also brings the mask rows and row offsets) */
    int32_t fill_stage_entries;    /* kept windows per staging block: a round with more takes passes */
} icv_pack_info;
int icv_pack_geometry(int32_t n_windows, icv_pack_info *h_info);

/* Step 5b fused with the packing (the public tl.infercnv path: X_cnv leaves the GPU as CSR and the dense thresholded
 * matrix is never needed): same decision as icv_apply_threshold, but `out` (the UN-thresholded x_res of
 * icv_infercnv_smooth / icv_infercnv_run with ICV_FLAG_NO_APPLY) is left untouched; the kept entries
 * (|x| >= thr in float64, x != 0; NaN kept) are recorded as bits, `mask` = n_rows x n_words uint64 with
 * n_words = ceil(n_windows / 64), and counted into `row_nnz`.  `thr` NULL = no threshold (dynamic_threshold=None).
 * icv_row_offsets turns row_nnz into indptr, icv_csr_fill_masked then packs indices / values at indptr[row]: the
 * public path's three calls, nothing is read back.  x_res is read twice in total and never rewritten.
 * Both passes stream x_res through an LDS ring (one persistent workgroup per CU, LDS-DMA loader wavefronts:
 * k_thr_mask_ring / k_csr_fill_ring, csrc/icv_kernel_pack.hpp) when its rows are 16-byte aligned (ldo a multiple of 4)
 * and hold 256 .. 2 048 windows (four rows a round through 160 KB of LDS); other shapes run one workgroup / wavefront
 * per row.  The streamed mask pass needs 24 * n_rows bytes of temporary device memory (stream-ordered) when `thr` is
 * given. */
int icv_threshold_mask(icv_plan_t plan, const icv_matrix *m, const void *ref_lo, const void *ref_hi,
                       double lfc_clip, int32_t flags, const float *out, int64_t ldo, const double *cell_median,
                       const double *thr, int64_t chunksize, int64_t row_phase, uint64_t *mask,
                       int64_t *row_nnz, void *stream);
int icv_csr_fill_masked(const float *x, int64_t n_rows, int32_t n_cols, int64_t ld, const uint64_t *mask,
                        const int64_t *indptr, int32_t *indices, double *data, void *stream);
/* the prefix sum between the two: indptr[0] = 0, indptr[r + 1] = row_nnz[0] + ... + row_nnz[r] (device arrays; two
 * launches over blocks of 4 096 rows, 8 bytes of temporary device memory per block) */
int icv_row_offsets(const int64_t *row_nnz, int64_t n_rows, int64_t *indptr, void *stream);

/* ---- ithcna / ithgex (tl/_scores.py:77-221) -------------------------------------------------
 * Interquartile range of all n x n entries of np.corrcoef(x) for one group of cells: x is a dense
 * float32 n x k matrix in HBM (rows = cells).  Rows are centred / scaled with float64 statistics, the
 * Gram matrix is computed with fp32 MFMA tiles, the percentiles (numpy "linear" method) from exactly
 * selected order statistics.  Synchronous (the selection reads counters back); *h_iqr is a host double.
 * Needs 4*n*(n + k) bytes of temporary device memory. */
int icv_corr_iqr(const float *x, int64_t n, int32_t k, int64_t ld, double *h_iqr, void *stream);

/* ---- cell-level hierarchical clustering behind the heatmap dendrogram (BASELINE.json config 5) ----
 * No call site in the reference (scanpy's `dendrogram=True` of sc.pl.heatmap, forwarded by
 * pl/_chromosome_heatmap.py:74-85, clusters category means); the oracle is scipy pdist + linkage("ward").
 *
 * icv_pairwise_sqeuclidean: out[(i - row_begin)*ldo + j] = ||x_i - x_j||^2 for row_begin <= i < row_end and
 * all 0 <= j < n (float32; the full symmetric n x n matrix with a zero diagonal for row range [0, n); a row
 * block is what one GPU of a row-sharded job computes).  x is a dense float32 n x d matrix in HBM; columns are
 * centred first (translation invariant), the contraction runs on fp32 MFMA tiles.  Needs 4*n*d + 8*n bytes
 * of temporary device memory.
 *
 * icv_ward_linkage: Ward linkage of the n points whose squared distances are in dist_sq (n x n float32 in
 * HBM, symmetric, row stride ld >= n; OVERWRITTEN).  spare_columns != 0: the caller also hands over columns
 * [n, ld) of every row as scratch (see "Column layout" below; ld % 4 == 0 and ld >= n + (n + 1) / 2 required, else
 * ICV_ERR_INVALID); 0: nothing outside the n x n block is touched, whatever the stride (dist_sq may be a column
 * slice of a wider buffer).  h_linkage is a HOST array of (n-1) x 4 doubles in scipy's linkage-matrix
 * format (cluster ids, height, size; rows sorted by height).  Synchronous; *h_rounds (optional) returns
 * the number of reciprocal-nearest-neighbour rounds.  ICV_ERR_INVALID if a distance is NaN. */
int icv_pairwise_sqeuclidean(const float *x, int64_t n, int32_t d, int64_t ld, int64_t row_begin, int64_t row_end,
                             float *out, int64_t ldo, void *stream);
int icv_ward_linkage(float *dist_sq, int64_t n, int64_t ld, int32_t spare_columns, double *h_linkage,
                     int32_t *h_rounds, void *stream);

/* The same two steps for a distance matrix SHARDED by rows over several GPUs (one process per GPU; the exchanges
 * between the calls are the caller's: infercnvpy_amd/dist.py does them with torch.distributed over RCCL).
 * Rows are owned in super-rows of ICV_SUPER_ROWS rows.
 *
 * icv_pairwise_sqeuclidean_tiles: this rank's share of the upper-triangular super-tiles (ICV_SUPER_ROWS x
 * ICV_SUPER_ROWS outputs each; x = ALL n points, resident).  Tile k covers rows row0[k].. and columns col0[k]..
 * (multiples of ICV_SUPER_ROWS, col0 >= row0); it is written to dir + dir_off[k] (row stride ld_dir) and, for the
 * part strictly above the diagonal, transposed to mir + mir_off[k] (row stride ld_mir): the rank writes its own
 * rows directly and the mirror blocks into the buffer that travels to the owners of those rows.  All arrays of
 * length n_tiles are HOST arrays.  Values are bit-identical to icv_pairwise_sqeuclidean's. */
#define ICV_SUPER_ROWS 1024
int icv_pairwise_sqeuclidean_tiles(const float *x, int64_t n, int32_t d, int64_t ld, int32_t n_tiles,
                                   const int32_t *h_row0, const int32_t *h_col0, const int64_t *h_dir_off,
                                   const int64_t *h_mir_off, float *dir, int64_t ld_dir, float *mir, int64_t ld_mir,
                                   void *stream);

/* Column layout of the Ward rounds (both entry points; chosen by the caller's spare_columns argument, never
 * inferred from the stride).  With spare columns -- a row stride that leaves at least n / 2 of them
 * (ld >= n + (n + 1) / 2, ld % 4 == 0) -- a merged cluster keeps its row but moves to a NEW column: the clusters
 * merged in a round take consecutive columns of the spare region, so that the update of every other row is one
 * contiguous strip instead of one 4-byte write per 128-byte line; the alive columns are compacted in place when
 * the region is full (such a matrix must be 16-byte aligned).  Without spare columns the columns are updated in
 * place.  Results are identical either way, bit for bit.
 *
 * Step-wise Ward rounds on a row-sharded matrix.  Every rank creates the same state (the bookkeeping is replicated
 * and deterministic); h_sr_local[g] = local super-row index of global super-row g on THIS rank (0 .. k-1) or -1
 * (NULL: all rows are local); ld = row stride of the local matrix, the same in every later call.  One round:
 *   icv_ward_merge     rows merged in the previous round, by their owners: new row, its nearest neighbour;
 *                      h_pslot[p] = row of `stage` holding the partner row of merge p (received from its owner) or
 *                      -1 if the partner is stored locally; scatter != 0: also update the other local rows
 *                      (single-GPU form; sharded callers use gather / exchange / scatter instead)
 *   icv_ward_gather    out[q][k] = entry of local row d_rows[q] (a new row) for the cluster of slot d_slots[k]:
 *                      the columns another rank needs, in the order of ITS local rows (device index arrays)
 *   icv_ward_scatter   the update of the local rows that did not merge from the n_pairs new rows v[q][local row]
 *                      (row stride ldv); v[q] belongs to merge h_vrow_p[q] of the round (a permutation)
 *   icv_ward_scan      nearest neighbour of the local rows whose cached neighbour merged or died
 *   icv_ward_pack_nn / icv_ward_unpack_nn   the round's (neighbour, distance) results, n_pairs + n_act entries in
 *                      list order, zero where another rank owns the row: all-reduce(SUM) them in between
 *   icv_ward_pairs     reciprocal pairs of the round (replicated); compacts the local rows first when the column
 *                      layout asks for it; h_counts = {n_live, n_merges, n_pairs, n_act} (synchronises the
 *                      stream); all_active != 0: list every live row for the next scan (the pass after a round
 *                      without a pair; it is not counted in icv_ward_finish's h_rounds)
 *   icv_ward_round_pairs  slots (i kept, j absorbed) of the pairs just found, HOST arrays of n_pairs
 * until n_live == 1; icv_ward_finish writes the linkage matrix as icv_ward_linkage does.  One in-flight call per
 * state. */
typedef struct icv_ward_s *icv_ward_t;
int icv_ward_create(int64_t n, const int32_t *h_sr_local, int32_t n_super, int32_t super_shift, int64_t ld,
                    int32_t spare_columns, icv_ward_t *out, void *stream);
void icv_ward_destroy(icv_ward_t w);
int icv_ward_merge(icv_ward_t w, float *d_local, int64_t ld, const float *stage, int64_t ld_stage,
                   const int32_t *h_pslot, int32_t scatter, void *stream);
int icv_ward_gather(icv_ward_t w, const float *d_local, int64_t ld, const int64_t *d_rows, int32_t n_rows,
                    const int32_t *d_slots, int32_t n_slots, float *out, int64_t ldo, void *stream);
int icv_ward_scatter(icv_ward_t w, float *d_local, int64_t ld, const float *v, int64_t ldv, const int32_t *h_vrow_p,
                     int32_t n_v, void *stream);
int icv_ward_scan(icv_ward_t w, const float *d_local, int64_t ld, void *stream);
int icv_ward_pack_nn(icv_ward_t w, int32_t *d_nn, float *d_dmin, void *stream);
int icv_ward_unpack_nn(icv_ward_t w, const int32_t *d_nn, const float *d_dmin, void *stream);
int icv_ward_pairs(icv_ward_t w, float *d_local, int64_t ld, int32_t all_active, int32_t *h_counts /* 4 */,
                   void *stream);
int icv_ward_round_pairs(icv_ward_t w, int32_t *h_i, int32_t *h_j);
int icv_ward_finish(icv_ward_t w, double *h_linkage, int32_t *h_rounds);

/* ---- cnv_score (tl/_scores.py:65-68): per-row sum of |x| in float64 ----------------------- */
int icv_row_abs_sum(const float *x, int64_t n_rows, int32_t n_cols, int64_t ld, double *row_sum,
                    void *stream);

/* the same on a CSR X_cnv (values float32 or float64, `indptr` n_rows + 1 int64 offsets into `data`): only the
 * stored entries are read, nothing is densified */
int icv_csr_row_abs_sum(const void *data, int32_t dtype, const int64_t *indptr, int64_t n_rows, double *row_sum,
                        void *stream);

/* per-group sums of per-cell values (cnv_score: score[g] = sum_g(row_sum) / (n_g * n_windows), tl/_scores.py:65-68):
 * sums[g] = sum of values[i] with group[i] == g (device int32 labels 0 .. n_groups-1; others are ignored), counts[g] =
 * how many.  Fixed summation order (one workgroup per group, strided partial sums + tree): the same bits for host and
 * device-resident X_cnv. */
int icv_group_sums(const double *values, const int32_t *group, int64_t n, int32_t n_groups, double *sums,
                   int64_t *counts, void *stream);

/* ---- device-resident CSR (a user-built device matrix as adata.X; X_cnv as tl.infercnv leaves it in HBM) ---------
 * icv_csr_check: the matrix is what the kernels expect -- offsets non-decreasing and inside [0, capacity] (capacity =
 * entries the index / value buffers hold), column indices inside [0, n_cols), ascending and unique within every row
 * (the host path gets this from scipy's canonical format; reference tl/_infercnv.py:115-116).  ICV_ERR_INVALID with
 * the defect in icv_last_error() otherwise.  Synchronises the stream (one flag is read back).
 * icv_csr_densify: out[q * ldo + c] = value of row rows[q] (device int64 list; NULL: rows 0 .. n_sel-1), column c, as
 * float32 -- the dense tile the fp32 MFMA contractions read (icv_corr_iqr for tl.ithcna, tl/_scores.py:197-213;
 * icv_pairwise_sqeuclidean for config 5); `data` float32 or float64. */
int icv_csr_check(const int64_t *indptr, const int32_t *indices, int64_t n_rows, int32_t n_cols, int64_t capacity,
                  void *stream);
int icv_csr_densify(const void *data, int32_t dtype, const int64_t *indptr, const int32_t *indices, const int64_t *rows,
                    int64_t n_sel, int32_t n_cols, float *out, int64_t ldo, void *stream);

/* ---- tl.pca (reference tl/__init__.py:33-75): the two passes over X_cnv ---------------------------------------------
 * icv_gram_f64: G (n_cols x n_cols, row stride ldg) = X^T X of the rows `m` describes (dense or CSR, float32 or
 * float64; the row range is the matrix's, as everywhere), summed in float64 with v_mfma_f64_16x16x4_f64; accumulate != 0
 * adds to G, 0 overwrites it.  G comes out bitwise symmetric.  `panel`: caller-owned device scratch of at least
 * (n_rows rounded up to 32) x panel_ld elements of panel_dtype, panel_ld >= n_cols rounded up to 64: the rows are
 * densified into it first.  A float32 panel rounds the values to float32: choose it only for float32-exact values
 * (float32 input, or X_cnv's float64 widenings of float32 numbers); products of float32 numbers are exact in float64.
 * The cells are summed in blocks of ICV_GRAM_BLOCK rows, each block's partial tile is added to G in row order with no
 * atomics: two calls give the same bits, and G summed over several calls equals one call over all rows bit for bit
 * when every call but the last covers a multiple of ICV_GRAM_BLOCK rows.  No synchronisation.
 * icv_project: out[q * ldo + c] = sum over row q's entries (stored order; a dense row's nonzero elements in column
 * order, so both formats give the same bits) of x * v[col * k + c], float64, minus shift[c] when `shift` is not NULL;
 * written as out_dtype (ICV_F32 / ICV_F64).  v: n_cols x k row-major float64 (device), shift: k float64 (device). */
#define ICV_GRAM_BLOCK 8192
int icv_gram_f64(const icv_matrix *m, int32_t panel_dtype, void *panel, int64_t panel_ld, double *g, int64_t ldg,
                 int32_t accumulate, void *stream);
int icv_project(const icv_matrix *m, const double *v, int32_t k, const double *shift, int32_t out_dtype, void *out,
                int64_t ldo, void *stream);

/* ---- pp.neighbors (reference pp/__init__.py:8-43; csrc/icv_knn.hpp) ------------------------------------
 * The EXACT k - 1 nearest other rows of every row of x (n x d float32, row stride ld; 2 <= k <= min(n, 64),
 * 1 <= d <= 256, n up to 2^30 by the index types):
 *   d2(i, j) = float64 sum over the columns, in order, no fused multiply-add, of (double(x_ic) - double(x_jc))^2;
 *   row i's neighbours are the j != i with the smallest (d2, j), listed in that order in knn_idx[i * (k - 1) + r]
 *   (int32) with knn_dist = float32(sqrt(d2)).  A pure function of x.
 * Stages: column-centred float32 copies; an fp32 MFMA sweep that keeps, per row and column part, the k - 1 + 8 smallest
 * LOWER BOUNDS of d2 (the n x n matrix is never stored); float64 re-ranking of those candidates; a certificate per
 * row (every cell that is not a candidate is provably farther than the (k-1)-th neighbour); the rows that fail it go
 * through an exact kernel against all n cells.  *n_exact (host, optional) = number of such rows: correctness does
 * not depend on it, speed does.  stage_ms (host, optional): float[4] = milliseconds of centring, sweep, re-ranking,
 * exact kernel.  The call synchronises the stream once (it reads the count of uncertified rows).
 * workspace: caller-owned device buffer of icv_knn_workspace(n, d, k) bytes, linear in n: per cell 4 DP (the centred
 * copy, DP = d rounded up to 64 / 128 / 256) + 4 (norm) + parts * (8 (k + 7) + 8) (candidates and bounds; parts = 1
 * above 131 072 cells, up to 16 for small n) + 4 (row list), n rounded up to 128. */
int icv_knn_workspace(int64_t n, int32_t d, int32_t k, int64_t *bytes);
int icv_knn(const float *x, int64_t n, int32_t d, int64_t ld, int32_t k, void *workspace, int32_t *knn_idx,
            float *knn_dist, int32_t *n_exact, float *stage_ms, void *stream);
/* UMAP's smooth_knn_dist + membership strengths on the stored float32 distances of icv_knn (rows ascending), float64,
 * one lane per row: rho[i] = smallest positive distance (0: none); sigma[i] by the bisection of DESIGN.md 4.9 rule 5
 * with its floor (the mean over ALL distances is summed in a fixed order: rows in order per thread of one workgroup,
 * then a tree); weights[i * (k - 1) + r] = 1 where dist - rho <= 0, else exp(-(dist - rho) / sigma).
 * 8 (n + 1) bytes of temporary device memory (stream-ordered).  No synchronisation. */
int icv_knn_fuzzy(const float *knn_dist, int64_t n, int32_t k, double *rho, double *sigma, double *weights,
                  void *stream);
/* C = A + A^T - A o A^T (A = the weights at the columns knn_idx) as canonical CSR, float32, entries that round to 0
 * not stored.  Two calls around icv_row_offsets: _count writes row_nnz[n] (integer atomics), _fill writes
 * indices / data for the nnz = indptr[n] entries (any fill order, then every row sorted by column: the result does
 * not depend on scheduling).  _fill: 4 n + 8 nnz bytes of temporary device memory.  No synchronisation. */
int icv_knn_symmetrize_count(const int32_t *knn_idx, const double *weights, int64_t n, int32_t k, int64_t *row_nnz,
                             void *stream);
int icv_knn_symmetrize_fill(const int32_t *knn_idx, const double *weights, int64_t n, int32_t k,
                            const int64_t *indptr, int64_t nnz, int32_t *indices, float *data, void *stream);
/* every CSR row's (column, value) pairs by ascending column (distinct columns per row; out of place) */
int icv_knn_sort_rows(const int64_t *indptr, int64_t n, const int32_t *cols_in, const float *vals_in, int32_t *cols,
                      float *vals, void *stream);

/* ---- tl.leiden: deterministic Leiden of a symmetric weighted graph, every phase on the device ------
 * icv_leiden_quantise validates the CSR graph (rule 1: rows strictly ascending, finite, non-negative, no diagonal,
 * symmetric pattern and values; each violation ICV_ERR_INVALID) and writes the integer graph of rule 2 (float32
 * rounding, w = rint(v 2^32), entries with w = 0 dropped): q_indptr (n + 1), q_indices / q_weights (capacity nnz).
 * result (host): [0] stored entries kept, [1] 2m = sum of the weights.  dtype: ICV_F32 / ICV_F64 of data.
 * icv_leiden_iteration runs ONE iteration (local moving, refinement, aggregation, level by level) from the partition
 * in labels (device, int32 n, ids in [0, n)) and writes the new one there (ids in [0, n), not renumbered).  gom =
 * resolution / double(2m); seed = random_state; trace (host, 3 * 64 int32) receives per level (vertices, rounds of
 * local moving, rounds of refinement), *n_levels the count, *n_moves the local-moving moves of all levels (0: the
 * iteration changed nothing), *bound_reached whether a bound of rule 5 ended a phase.  stage_ms (host, optional):
 * float[4] = local moving, refinement, aggregation, the rest.  The host reads two scalars per round.  Rows of any
 * length: up to 512 entries a wavefront combines the row in LDS, longer rows take a workgroup and a table in the
 * workspace.
 * workspace: icv_leiden_workspace(n, nnz) bytes = 128 n + 80 nnz + O(1) (two aggregate graphs, the per-vertex
 * arrays, the sort buffers, 24 nnz of tables for the long rows).  Outside it, from the stream's memory pool: the
 * temporaries of the sort / segmented-sum / scan primitives, 8 (n + nnz) in icv_leiden_quantise, 36 n in
 * icv_leiden_renumber.
 * icv_leiden_sums: e[c] = weight inside label c (both directions), K[c] = its strength (device int64, n each).
 * icv_leiden_renumber: rule 6 (decreasing size, ties by the smallest member); *n_communities on the host. */
int icv_leiden_workspace(int64_t n, int64_t nnz, int64_t *bytes);
int icv_leiden_quantise(const int64_t *indptr, const int32_t *indices, const void *data, int32_t dtype, int64_t n,
                        int64_t nnz, int32_t use_weights, int64_t *q_indptr, int32_t *q_indices, int64_t *q_weights,
                        int64_t *result, void *stream);
int icv_leiden_iteration(const int64_t *indptr, const int32_t *indices, const int64_t *weights, int64_t n, int64_t nnz,
                         double gom, uint64_t seed, int32_t iteration, int32_t *labels, void *workspace, int32_t *trace,
                         int32_t *n_levels, int64_t *n_moves, int32_t *bound_reached, float *stage_ms, void *stream);
int icv_leiden_sums(const int64_t *indptr, const int32_t *indices, const int64_t *weights, int64_t n,
                    const int32_t *labels, int64_t *e, int64_t *K, void *stream);
int icv_leiden_renumber(const int32_t *labels, int64_t n, int32_t *out, int32_t *n_communities, void *stream);

/* ---- tl.umap: deterministic UMAP layout of a symmetric fuzzy graph ---------------------------------
 * icv_umap_epochs runs the epochs [epoch_begin, epoch_end) of an n_epochs schedule on the positions y (device float32,
 * n x n_components row-major, in / out), one kernel launch per epoch.  The schedule is stateless (rule 2), so any
 * range may be run alone and [0, E) in one call equals E calls of one epoch bit for bit.  The graph is a canonical CSR
 * (indptr int64 n + 1 trusted, indices int32, data float32; rule 1: rows strictly ascending, finite, non-negative, no
 * diagonal, symmetric pattern and values; each violation ICV_ERR_INVALID, checked in every call before y is touched).
 * n_components: 2 or 3.  a, b > 0; gamma >= 0; 0 <= negative_sample_rate <= 64; initial_alpha >= 0; seed =
 * random_state.  Every row sum is an int64 sum of contributions rounded to 2^-32: the result is a pure function of
 * the arguments.  Rows up to 512 entries take a wavefront, longer rows a workgroup (the same launch).
 * stage_ms (host, optional): float[2] = validation, epochs.  The host reads three scalars after the validation; the
 * epochs are enqueued without synchronisation (with stage_ms the call waits for them).
 * workspace: icv_umap_workspace(n, nnz, n_components) bytes = 4 n n_components + 4 (n + 1) + 64, each part rounded up
 * to 256 (the second position buffer, the list of the long rows, three scalars); nnz only bounds the arguments. */
int icv_umap_workspace(int64_t n, int64_t nnz, int32_t n_components, int64_t *bytes);
int icv_umap_epochs(const int64_t *indptr, const int32_t *indices, const float *data, int64_t n, int64_t nnz,
                    int32_t n_components, double a, double b, double gamma, int32_t negative_sample_rate,
                    double initial_alpha, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, uint64_t seed,
                    float *y, void *workspace, float *stage_ms, void *stream);

/* ---- tl.tsne: deterministic t-SNE with the exact repulsion ---------------------------------------------
 * icv_tsne_affinities: rule 2 on the stored float32 distances of icv_knn (n x k, nearest first; 1 <= k <= 63;
 * 0 < perplexity < k), float64, one lane per row: beta[i] by the fixed bisection (at most 64 bracket steps, then 64
 * halvings, no early exit) on the entropy of exp(-beta (d_r^2 - d_0^2)) with the library's WRITTEN exponential, and the
 * conditional affinities cond[i * k + r] (a row of equal distances: beta 1, cond 1 / k).  No synchronisation.
 * icv_tsne_symmetrize_count / _fill: W = A + A^T (A = cond at the columns knn_idx) as canonical CSR, float32, entries
 * that round to 0 not stored; shapes, temporary memory and the two-call protocol of icv_knn_symmetrize_* (whose k
 * counts the cell itself: here k is the number of columns of knn_idx, 1 <= k <= 63). */
int icv_tsne_affinities(const float *knn_dist, int64_t n, int32_t k, double perplexity, double *beta, double *cond,
                        void *stream);
int icv_tsne_symmetrize_count(const int32_t *knn_idx, const double *cond, int64_t n, int32_t k, int64_t *row_nnz,
                              void *stream);
int icv_tsne_symmetrize_fill(const int32_t *knn_idx, const double *cond, int64_t n, int32_t k, const int64_t *indptr,
                             int64_t nnz, int32_t *indices, float *data, void *stream);
/* icv_tsne_iterations runs the iterations [iter_begin, iter_end) of rules 4-6 on the caller's state (device float32,
 * n x n_components row-major, in / out): positions y, last updates `update` (zeros before iteration 0) and gains (ones
 * before iteration 0).  Two kernel launches per iteration: the repulsion over all ordered pairs, and the attraction
 * over the stored entries with the gradient step.  The schedule is stateless (exaggeration early_exaggeration and
 * momentum 0.5 for t < exaggeration_iters, then 1 and 0.8), so any range may be run alone and [0, T) in one call
 * equals T calls of one iteration bit for bit; no early stopping.  The graph W is a canonical CSR (indptr int64 n + 1
 * trusted, indices int32, data float32: rows strictly ascending, finite, 0 <= value <= 2, no diagonal, symmetric
 * pattern and values; each violation ICV_ERR_INVALID, checked in every call before the state is touched); a row above
 * 2^22 entries is ICV_ERR_UNSUPPORTED.  n_components: 2 or 3.  early_exaggeration, learning_rate finite and > 0.
 * Every sum over pairs or entries is an exact int64 sum: the result is a pure function of the arguments.
 * stage_ms (host, optional): float[2] = validation, iterations.  The host reads three scalars after the validation;
 * the iterations are enqueued without synchronisation (with stage_ms the call waits for them).
 * workspace: icv_tsne_workspace(n, nnz, n_components) bytes = 3 x 4 n n_components (the second state buffers)
 * + 2 x (8 n + 8 n n_components + 256) (two sets of integer accumulators) + 4 ceil(n / 256) (tickets) + 4 (n + 1)
 * (the long rows) + 256, each part rounded up to 256; nnz only bounds the arguments. */
int icv_tsne_workspace(int64_t n, int64_t nnz, int32_t n_components, int64_t *bytes);
int icv_tsne_iterations(const int64_t *indptr, const int32_t *indices, const float *data, int64_t n, int64_t nnz,
                        int32_t n_components, double early_exaggeration, int32_t exaggeration_iters,
                        double learning_rate, int32_t iter_begin, int32_t iter_end, float *y, float *update,
                        float *gains, void *workspace, float *stage_ms, void *stream);

/* ---- tl.cnv_states: loss / neutral / gain calls of X_cnv by a Viterbi chain per chromosome -------------
 * The matrix m (dense or CSR, float32 or float64, device pointers; a CSR with unique column indices inside
 * [0, n_cols) in every row) is read as float64, an entry that is not stored is 0.0.
 * icv_states_rowsq: rowsq[i] = the float64 sum of v v over row i's stored entries in stored order (every element of a
 * dense row), one sequential sum per row; *nonfinite (device int32) is set to 0 and then to 1 where a value is not
 * finite.  No synchronisation.
 * icv_states_viterbi: rules 2-5 of the contract.  chr_start (device int32, n_chr + 1 ascending window numbers from 0 to
 * n_cols) bounds the chains; amplitude > 0, h = 1 / (2 sigma^2) > 0, stay = log(1 - p) and sw = log(p / 2) are the
 * host's doubles, all finite.  states (device int8, n_rows x n_cols row-major, no padding) receives -1 / 0 / +1,
 * nonneutral[i] (device int32) the number of windows of row i that are not 0.  One wavefront per row, 9 bytes of LDS
 * per window: 1 <= n_cols <= ICV_STATES_MAX_WINDOWS (ICV_ERR_INVALID beyond).  The result is a pure function of the
 * arguments.  No synchronisation.
 * icv_states_fraction: fraction[i] (device float64) = nonneutral[i] / n_cols, the correctly rounded quotient of the two
 * integers (what the host's float64 division gives).  No synchronisation. */
#define ICV_STATES_MAX_WINDOWS 16384
int icv_states_rowsq(const icv_matrix *m, double *rowsq, int32_t *nonfinite, void *stream);
int icv_states_viterbi(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, double amplitude, double h,
                       double stay, double sw, int8_t *states, int32_t *nonneutral, void *stream);
int icv_states_fraction(const int32_t *nonneutral, int64_t n_rows, int32_t n_cols, double *fraction, void *stream);

/* ---- tl.cnv_segments: segment tables of the int8 call matrix of tl.cnv_states ------------------------------
 * states (device int8, n_rows x n_cols row-major, no padding, any alignment) holds -1 / 0 / +1; chr_start (device int32,
 * n_chr + 1 ascending window numbers from 0 to n_cols, 1 <= n_chr <= n_cols) bounds the chromosomes.  Window t starts a
 * run iff states[i,t] != 0 and (t is a chromosome start or states[i,t-1] differs); it ends one iff states[i,t] != 0 and
 * (t + 1 == n_cols or t + 1 is a chromosome start or states[i,t+1] differs).  Everything is integer arithmetic: the
 * results are a pure function of the arguments.  n_cols has no limit below int32.  No synchronisation anywhere.
 * icv_segments_count: counts[i] (device int64) = the runs of row i; *bad (device int32) is set to 0 and then to 1 where a
 * value is not -1 / 0 / +1.  icv_row_offsets turns counts into offsets (n_rows + 1).
 * icv_segments_fill: segment offsets[i] + k (row i's k-th run, by start) gets seg_row (int64), seg_start, seg_end
 * (int32, exclusive) and seg_state (int8); the four tables hold n_segments = offsets[n_rows] entries and nothing is
 * written outside them.
 * icv_state_votes: rows (device int64, n_listed row numbers, sorted by group) and group_ptr (device int64, n_groups + 1
 * ascending positions from 0 to n_listed) list the rows of every group; loss / gain (device int32, n_groups x n_cols) are
 * zeroed and receive the number of listed rows of the group with -1 / +1 at the window (integer atomic adds).  A row
 * number outside [0, n_rows) is skipped; *bad as above, for the rows that are listed.  n_groups has no limit.
 * icv_state_consensus: consensus (device int8, n_groups x n_cols) = +1 where gain >= need[g] and gain > loss, -1 where
 * loss >= need[g] and loss > gain, else 0 (need: device int32 per group).
 * icv_segments_support: for every segment of the consensus matrix (the tables of icv_segments_fill, seg_row = the group)
 * cells_min (int32) / cells_sum (int64) = the minimum / the sum over its windows of the winning state's count; a segment
 * outside the n_groups x n_cols tables gets 0 / 0. */
int icv_segments_count(const int8_t *states, int64_t n_rows, int32_t n_cols, const int32_t *chr_start, int32_t n_chr,
                       int64_t *counts, int32_t *bad, void *stream);
int icv_segments_fill(const int8_t *states, int64_t n_rows, int32_t n_cols, const int32_t *chr_start, int32_t n_chr,
                      const int64_t *offsets, int64_t n_segments, int64_t *seg_row, int32_t *seg_start, int32_t *seg_end,
                      int8_t *seg_state, void *stream);
int icv_state_votes(const int8_t *states, int64_t n_rows, int32_t n_cols, const int64_t *rows, int64_t n_listed,
                    const int64_t *group_ptr, int64_t n_groups, int32_t *loss, int32_t *gain, int32_t *bad, void *stream);
int icv_state_consensus(const int32_t *loss, const int32_t *gain, const int32_t *need, int64_t n_groups, int32_t n_cols,
                        int8_t *consensus, void *stream);
int icv_segments_support(const int64_t *seg_row, const int32_t *seg_start, const int32_t *seg_end, const int8_t *seg_state,
                         int64_t n_segments, const int32_t *loss, const int32_t *gain, int64_t n_groups, int32_t n_cols,
                         int32_t *cells_min, int64_t *cells_sum, void *stream);

/* ---- tl.cnv_posteriors and tl.cnv_states_filter: posteriors of the model of tl.cnv_states -------------------
 * icv_posterior_chains: forward-backward along every chromosome of every row of m (the matrix, chr_start, amplitude and
 * h as for icv_states_viterbi; ps = 1 - p and pw = p / 2 are the host's doubles for a p in (0, 1), pw a normal float64).
 * Emissions b(s) = exp_(e_s - max e) with e_s of 4.13 and the written exponential of 4.12; forward al_t = u_t / c_t with
 * u_t(s) = (((al(0) A(0,s)) + (al(1) A(1,s))) + (al(2) A(2,s))) b_t(s), c_t = (u(0) + u(1)) + u(2); backward
 * be_t(r) = (((A(r,0) g(0)) + (A(r,1) g(1))) + (A(r,2) g(2))) / c_{t+1} with g = b_{t+1} be_{t+1}; the posterior is
 * (al_t be_t) / ((w(0) + w(1)) + w(2)).  Float64, no fused multiply-add, every division correctly rounded: the result is a
 * pure function of the arguments.  neutral (device float64, n_rows x n_cols row-major, no padding) receives P(neutral);
 * loss and gain are either both null or receive P(loss) and P(gain).  One wavefront per row, 32 bytes of LDS per window:
 * 1 <= n_cols <= ICV_POSTERIOR_MAX_WINDOWS (ICV_ERR_INVALID beyond).  No synchronisation.
 * icv_states_filter: states (device int8) and p_neutral (device float64), both n_rows x n_cols row-major without padding;
 * runs as in 4.14.  With q_t = int64(rint(p_neutral[i,t] 2^40)), a run [s, e) is reset to 0 in filtered (device int8,
 * n_rows x n_cols) iff double(sum of its q_t) / (double(e - s) 2^40) > max_p_normal (in [0, 1]); every other window is
 * copied.  nonneutral[i] / removed[i] (device int32) = the windows of filtered's row i that are not 0 / the runs of row i
 * that were reset.  *bad (device int32) is set to 0 and then to 1 where a state is not -1 / 0 / +1 or a posterior is not a
 * number in [0, 1].  Integer sums: a pure function of the arguments.  No row is held in LDS; n_cols <=
 * ICV_FILTER_MAX_WINDOWS keeps a run's sum inside int64 (ICV_ERR_UNSUPPORTED beyond).  No synchronisation. */
#define ICV_POSTERIOR_MAX_WINDOWS 4096
#define ICV_FILTER_MAX_WINDOWS 4194304
int icv_posterior_chains(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, double amplitude, double h,
                         double ps, double pw, double *neutral, double *loss, double *gain, void *stream);
int icv_states_filter(const int8_t *states, const double *p_neutral, int64_t n_rows, int32_t n_cols,
                      const int32_t *chr_start, int32_t n_chr, double max_p_normal, int8_t *filtered, int32_t *nonneutral,
                      int32_t *removed, int32_t *bad, void *stream);

/* ---- tl.cnv_states_fit: the E-step of the Baum-Welch fit of the model of tl.cnv_states ----------------------
 * icv_posterior_stats: forward-backward exactly as icv_posterior_chains (the same arguments, rules and bits of b, al_t,
 * c_t, be_t, z_t and gamma_t), reduced per row to stats[i] = (G, D, K) (device float64, n_rows x 3).  Per chromosome three
 * sums start at 0.0 and take their terms for t = T-1 down to 0: G += (gamma_t(0) + gamma_t(2));
 * D += (gamma_t(2) - gamma_t(0)) x_t; for t <= T-2, K += (st / c_{t+1}) / z_t with m(s) = (al_t(s) ps) g(s),
 * g = b_{t+1} be_{t+1} and st = (m(0) + m(1)) + m(2).  The row's G, D and K start at 0.0 and add the chromosome sums in
 * ascending chromosome order.  Float64, no fused multiply-add, no atomics: a pure function of the arguments.  One
 * wavefront per row, 32 bytes of LDS per window: 1 <= n_cols <= ICV_POSTERIOR_MAX_WINDOWS (ICV_ERR_INVALID beyond).  No
 * synchronisation. */
int icv_posterior_stats(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, double amplitude, double h, double ps,
                        double pw, double *stats, void *stream);

/* ---- tl.cnv_pseudobulk: the exact mean profile of every group of rows ---------------------------------------
 * icv_group_profiles: rows (device int64, n_listed row numbers, sorted by group) and group_ptr (device int64, n_groups + 1
 * ascending positions from 0 to n_listed) list the rows of every group, as for icv_state_votes; a row may stand in
 * several lists.  Stored values are used as float64; q = rint(v 2^shift), ties to even, as int64 (0 <= shift <= 40,
 * ICV_ERR_INVALID beyond; the caller keeps every stored magnitude below 2^10 and (rows of the largest group) 2^shift at
 * or below 2^52, so no sum leaves int64).  sum (device int64, n_groups x n_cols) and stored (device int32, the same
 * shape) are zeroed and receive the sum of q and the number of stored values != 0 of the group's listed rows at every
 * window: integer atomic adds, a pure function of the arguments.  -0.0 and a stored 0.0 add to neither.  CSR columns need
 * be neither sorted nor unique; a column outside [0, n_cols) is passed over.  *flags (device int32) is set to 0; bit 0 is
 * then set where a value that was read is not finite (it adds to neither table), bit 1 where a row number lies outside
 * [0, n_rows) (that row is skipped).  n_cols and n_groups have no limit.  No synchronisation.
 * icv_group_profiles_finish: with L = group_ptr[g + 1] - group_ptr[g], mean[g,w] = (double(sum) / double(L)) 2^-shift --
 * the conversion rounds to nearest even, the division is correctly rounded, the scaling exact -- and fraction[g,w] =
 * double(stored) / double(L) (device float64, n_groups x n_cols each); a group of no rows gets 0 in both. */
int icv_group_profiles(const icv_matrix *m, const int64_t *rows, int64_t n_listed, const int64_t *group_ptr,
                       int64_t n_groups, int32_t shift, int64_t *sum, int32_t *stored, int32_t *flags, void *stream);
int icv_group_profiles_finish(const int64_t *sum, const int32_t *stored, const int64_t *group_ptr, int64_t n_groups,
                              int32_t n_cols, int32_t shift, double *mean, double *fraction, void *stream);

/* ---- tl.cnv_correlation and tl.cnv_signal: the rows of a matrix against centred profiles ------------------
 * icv_profile_corr: m as for icv_states_viterbi (stored values are used as float64, an entry that is not stored is 0; CSR
 * columns ascending; a column outside [0, n_cols) is passed over).  profiles_t (device float64, n_cols x n_profiles
 * row-major: the n_profiles values of one window are contiguous) holds the centred profiles c_g = p_g - mean(p_g), s2
 * (device float64, n_profiles) their sums of squares; both are the host's doubles.  Per row i, sequentially over the
 * windows in ascending order and starting from +0.0: A += x, B += x x, D_g += x c_g[w], every product rounded before its
 * add (float64, no fused multiply-add); a term with x == 0 adds nothing, so a CSR and a dense form of one matrix give the
 * same bits.  a, b (device float64, n_rows) receive A and B, signal (the same shape) B / n_cols, and r (device float64,
 * n_rows x n_profiles row-major) r_ig = D_ig / sqrt(vx_i s2_g) with vx_i = B_i - (A_i A_i) / n_cols, clipped to
 * [-1, 1], NaN where vx_i <= 0 or s2_g == 0: each a correctly rounded operation, a pure function of the arguments.
 * n_profiles = 0 is allowed (profiles_t, s2 and r may be null) and gives a, b and signal alone.  *flags (device int32)
 * is set to 0; bit 0 is then set where a stored value is not finite.  n_cols has no limit and n_profiles none below
 * 64 x 65535 (ICV_ERR_UNSUPPORTED beyond).  No synchronisation.
 * icv_profile_corr_best: best_g[i] (device int32) = the lowest g with the largest r[i,g] that is no NaN and best_r[i]
 * (device float64) that value; -1 and NaN when the whole row is NaN or n_profiles = 0. */
int icv_profile_corr(const icv_matrix *m, const double *profiles_t, const double *s2, int64_t n_profiles, double *a,
                     double *b, double *signal, double *r, int32_t *flags, void *stream);
int icv_profile_corr_best(const double *r, int64_t n_rows, int64_t n_profiles, double *best_r, int32_t *best_g,
                          void *stream);

/* ---- tl.cnv_silhouette: exact silhouette widths of the labelled cells ---------------------------------------
 * The labelled cells are numbered by position: sorted by group, ascending row inside a group.  rows (device int64,
 * n_listed) maps a position to its row of x, a device row-major n_rows x n_comp matrix of dtype ICV_F32 / ICV_F64 with
 * ld elements between rows, 1 <= n_comp <= ICV_SILHOUETTE_MAX_COMPONENTS; values are used as float64.  A row number
 * outside [0, n_rows) is never read: its position counts as a cell at the origin.
 * icv_silhouette_sums: for the positions i in [i0, i1) (i0 a multiple of ICV_SILHOUETTE_TILE_I, i1 <= n_listed) and every
 * group g, sums[(i - i0) n_groups + g] (device int64; the entry clears it) = the int64 sum over the positions j of the
 * tiles of group g of rint(d_ij 2^shift), ties to even, where d_ij = sqrt(acc) and acc starts at +0.0 and takes
 * acc = acc + t t, t = x_ic - x_jc, over the components in ascending order (float64, every product rounded before its
 * add, the square root correctly rounded).  tiles (device int64, 3 x n_tiles row-major): first position, number of
 * positions (1 .. ICV_SILHOUETTE_TILE_J) and group of every tile; a tile that names a group outside [0, n_groups) or
 * positions outside [0, n_listed) is passed over.  chunk_ptr (device int32, n_chunks + 1 ascending tile numbers from 0 to
 * n_tiles): a workgroup takes ICV_SILHOUETTE_TILE_I positions i and the tiles of one chunk and adds one 64-bit integer
 * atomic per (i, run of tiles of one group), so the sums do not depend on the cut into tiles and chunks.  The components
 * pass through LDS in stages of ICV_SILHOUETTE_TILE_C.  0 <= shift <= ICV_SILHOUETTE_MAX_SHIFT; dist_exp: every d_ij is
 * below 2^dist_exp (the caller's bound; with shift + dist_exp <= 51 the rounding is one float64 addition, otherwise rint
 * and a conversion: the same integers).  The caller keeps every group sum below 2^62.  *flags (device int32) is NOT
 * cleared, so that the calls for the row slabs of one table share it: bit 0 is set where a value that was read is not
 * finite.  n_chunks <= 65535 (ICV_ERR_UNSUPPORTED beyond).  No synchronisation.
 * icv_silhouette_finish: group_ptr (device int64, n_groups + 1) holds the first position of every group.  For the
 * positions p in [i0, i1), with the sums of the same slab: mean(p, g) = double(sum) / (double(cnt) 2^shift), cnt =
 * n_g - 1 for p's own group and n_g otherwise (the conversion rounds to nearest even, the divisor is exact, the division
 * correctly rounded); a[p] = the own-group mean, 0.0 where the group is p alone; b[p] = the smallest mean over the other
 * groups that have cells and nearest[p] (device int32) the lowest group that attains it (0.0 and -1 where there is
 * none); s[p] = (b - a) / max(a, b), 0.0 where the own group is p alone or max(a, b) == 0.  s, a, b (device float64)
 * and nearest are indexed by position. */
#define ICV_SILHOUETTE_TILE_I 64
#define ICV_SILHOUETTE_TILE_J 64
#define ICV_SILHOUETTE_TILE_C 32
#define ICV_SILHOUETTE_MAX_COMPONENTS 256
#define ICV_SILHOUETTE_MAX_SHIFT 40
int icv_silhouette_sums(const void *x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const int64_t *rows,
                        int64_t n_listed, int64_t i0, int64_t i1, const int64_t *tiles, int64_t n_tiles,
                        const int32_t *chunk_ptr, int32_t n_chunks, int64_t n_groups, int32_t shift, int32_t dist_exp,
                        int64_t *sums, int32_t *flags, void *stream);
int icv_silhouette_finish(const int64_t *sums, int64_t i0, int64_t i1, const int64_t *group_ptr, int64_t n_groups,
                          int32_t shift, double *s, double *a, double *b, int32_t *nearest, void *stream);

/* ---- tl.cnv_kmeans: deterministic exact k-means of the representation -----------------------------------------
 * x is a device row-major n_rows x n_comp matrix of dtype ICV_F32 / ICV_F64 with ld elements between rows, n_rows >= 1,
 * 1 <= n_comp <= ICV_KMEANS_MAX_COMPONENTS; values are used as float64.  centres is a device float64 n_clusters x n_comp
 * table, 1 <= n_clusters <= ICV_KMEANS_MAX_CLUSTERS.  D(i, g) starts at +0.0 and takes acc = acc + t t, t = x_ic - c_gc,
 * over the components in ascending order (every product rounded before its add).  Shifts lie in
 * [0, ICV_KMEANS_MAX_SHIFT]; the caller chooses them so that no integer sum leaves int64 (DESIGN.md 4.27 rule 2).  *flags
 * (device int32) is never cleared: bit 0 is set where a value that was read is not finite, bit 1 where the seeding
 * weights of a draw add up to 0.  Every entry refuses a null pointer or an argument out of range with ICV_ERR_INVALID
 * before any GPU work.  No synchronisation.
 * icv_kmeans_seed_dist: for every row, mind[i] = D(i, centre) when first, otherwise the smaller of that and mind[i];
 * w[i] = rint(mind[i] 2^shift_f) as int64, ties to even; partials[j] = the sum of w over the rows
 * [j ICV_KMEANS_SEED_ROWS, + ICV_KMEANS_SEED_ROWS) (device int64, ceil(n_rows / ICV_KMEANS_SEED_ROWS) of them).  No atomics.
 * icv_kmeans_seed_pick: one workgroup.  t == 0: the row is z mod n_rows.  t > 0: W = the sum of partials, theta = z mod W
 * (unsigned 64-bit), the row is the first whose inclusive prefix sum of w in row order exceeds theta.  The row's values
 * become centres[t n_comp ..] and picks[t] (device int64) its number; W == 0 sets bit 1 of *flags and picks[t] = -1 and
 * leaves the centre as it is.
 * icv_kmeans_assign: labels[i] (device int32) = the lowest g that attains the smallest D(i, g), sqdist[i] that D;
 * stats (device int64, 2; the entry clears it): stats[0] = the int64 sum of rint(sqdist[i] 2^shift_f), stats[1] = the
 * number of rows whose label differs from the one found in labels before the call.
 * icv_kmeans_update: sums (device int64, n_clusters (n_comp + 1); the entry clears it): sums[g n_comp + c] = the int64 sum
 * of rint(x_ic 2^shift_e) over the rows with label g, sums[n_clusters n_comp + g] = their number.  A label outside
 * [0, n_clusters) is in no sum.  One workgroup per (ICV_KMEANS_UPDATE_ROWS rows, ICV_KMEANS_UPDATE_TILE_C components) sums
 * in LDS and adds one 64-bit atomic per non-zero sum, so the sums do not depend on the cut.
 * icv_kmeans_centres: centres[g, c] = double(sum) / (double(n_g) 2^shift_e) for every g with n_g > 0 (the conversions
 * round to nearest even, the divisor is exact, the division correctly rounded); the other centres stay. */
#define ICV_KMEANS_TILE_CELLS 256
#define ICV_KMEANS_TILE_CENTRES 16
#define ICV_KMEANS_TILE_C 32
#define ICV_KMEANS_MAX_COMPONENTS 256
#define ICV_KMEANS_MAX_CLUSTERS 256
#define ICV_KMEANS_MAX_SHIFT 40
#define ICV_KMEANS_SEED_ROWS 256
#define ICV_KMEANS_UPDATE_ROWS 1024
#define ICV_KMEANS_UPDATE_TILE_C 16
int icv_kmeans_seed_dist(const void *x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const double *centre,
                         int32_t first, int32_t shift_f, double *mind, int64_t *w, int64_t *partials, int32_t *flags,
                         void *stream);
int icv_kmeans_seed_pick(const void *x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const int64_t *w,
                         const int64_t *partials, int32_t t, int32_t n_clusters, uint64_t z, double *centres,
                         int64_t *picks, int32_t *flags, void *stream);
int icv_kmeans_assign(const void *x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const double *centres,
                      int32_t n_clusters, int32_t shift_f, int32_t *labels, double *sqdist, int64_t *stats, int32_t *flags,
                      void *stream);
int icv_kmeans_update(const void *x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const int32_t *labels,
                      int32_t n_clusters, int32_t shift_e, int64_t *sums, void *stream);
int icv_kmeans_centres(const int64_t *sums, int32_t n_clusters, int32_t n_comp, int32_t shift_e, double *centres,
                       void *stream);

/* ---- tl.cnv_changepoints: exact penalised least-squares segmentation of every chromosome of every row ---
 * icv_changepoint_levels: m and chr_start as for icv_states_viterbi (stored values are used as float64, an entry that is
 * not stored is 0.0; CSR columns need not be sorted; a column outside [0, n_cols) is passed over), except that n_cols has
 * no limit: one wavefront runs one (row, chromosome) and keeps 28 bytes of LDS per window of the chromosome, so every
 * chromosome has at most ICV_CHANGEPOINT_MAX_CHR_WINDOWS windows and n_rows x n_chr <= 2^31 - 1 (ICV_ERR_UNSUPPORTED
 * beyond).  Per row and chromosome with the values x_1 .. x_L: P_0 = Q_0 = +0.0, P_j = P_{j-1} + x_j,
 * Q_j = Q_{j-1} + x_j x_j; the cost of the segment (i, j] is c = (Q_j - Q_i) - (d d) / (double)(j - i) with d = P_j - P_i,
 * a c < 0.0 becomes 0.0; F_0 = 0.0 and F_j = the smallest ((F_i + c) + beta) over the i with (i == 0 or i >= min_windows)
 * and j - i >= min_windows, ties to the lowest i (i = 0 always counts for j = L; a j without such an i has F_j = +inf and
 * is never chosen); the backtrack from L gives the segments, each with the level (P_j - P_i) / (double)(j - i).  levels
 * (device float64, n_rows x n_cols) receives the level of every window's segment and starts (device uint8, the same
 * shape) 1 at the first window of every segment, 0 elsewhere.  Every operation is a correctly rounded float64 one in the
 * written order: a pure function of the arguments.  beta is finite and >= 0, min_windows >= 1.
 * icv_changepoint_diffsq: d[i] (device float64, n_rows) = the sum over the chromosomes in ascending order, from +0.0, of
 * each chromosome's sum, from +0.0 and in ascending order, of (x_{t+1} - x_t)^2 over its adjacent windows.
 * Both copy the n_chr + 1 starts to the host to size the launch (one synchronisation of the stream) and return
 * ICV_ERR_INVALID unless they ascend from 0 to n_cols with no chromosome above the cap. */
#define ICV_CHANGEPOINT_MAX_CHR_WINDOWS 4096
int icv_changepoint_levels(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, double beta, int32_t min_windows,
                           double *levels, uint8_t *starts, void *stream);
int icv_changepoint_diffsq(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, double *d, void *stream);

/* ---- tl.cnv_rank_groups: the exact doubled mid-rank sums of every group of rows in every window -----------
 * A value is what it is for icv_group_profiles: stored values are used as float64, an entry that is not stored is 0, a
 * stored 0.0 or -0.0 is the same 0; CSR columns need not be sorted but are unique within a row (a duplicate would be
 * ranked as a cell of its own); a column outside [0, n_cols) is passed over.  code (device
 * int32, n_rows) gives every row its group: a row with code < 0 is outside the population, the N others are ranked
 * against each other, N < ICV_RANK_MAX_CELLS so that N^3 fits an int64 (icv_rank_sums and icv_rank_finish return
 * ICV_ERR_INVALID beyond, before anything is launched).  All five enqueue on the stream and synchronise nothing.
 * icv_rank_count: stored (device int32, n_cols) is zeroed and receives per window the number of the population's values
 * that are neither 0 nor non-finite; *flags (device int32) is set to 0 and bit 0 is then set where a value of the
 * population is not finite.  n_cols has no limit.
 * The caller cuts the windows into consecutive tiles [w0, w0 + n_win) and forms seg_off (device int32, n_win + 1): the
 * exclusive prefix sum of stored over the tile, from 0; n_entries = seg_off[n_win] <= 2^31 - 1.
 * icv_rank_scatter: cursor (device int32, n_win) is zeroed; every counted value of the tile is written to a slot of its
 * window's segment of keys (device uint64, n_entries) and payload (device int32, n_entries): the key is the
 * order-preserving image of the float64 (bit pattern with the sign bit set for a positive value, all bits inverted for a
 * negative one), the payload the row's code.  The order inside a segment is arbitrary.  A value that finds its segment
 * full (the matrix is not the one that was counted) is dropped.
 * icv_rank_sort: keys_sorted / payload_sorted receive every segment sorted by key (rocprim's segmented radix sort; the
 * order of equal keys is arbitrary and nothing reads it).
 * icv_rank_sums: longest = the longest segment of the tile (it sizes the grid).  r2 (device int64) and cnt (device int32)
 * are n_codes x n_cols tables, tie (device int64) and neg (device int32) have n_cols elements; the caller zeroes all four
 * before the first tile.  For the entry at position p of its sorted segment, with [s, e) its run of equal keys and
 * z0 = n_pop - (segment length): 2r = s + e + 1, plus 2 z0 for a positive value, is added to r2[code, w] and 1 to
 * cnt[code, w] (a code outside [0, n_codes) adds nothing); the first entry of a run of c > 1 adds c^3 - c to tie[w];
 * neg[w] receives the number of negative values.  A run may have any length.  Integer atomic adds only: a pure function
 * of the arguments.
 * icv_rank_finish: after the last tile, for the first n_groups codes (n_cells, device int64, their sizes):
 * r2[g,w] += (n_cells[g] - cnt[g,w]) (2 neg[w] + z0 + 1) and tie[w] += z0^3 - z0 with z0 = n_pop - stored[w], the block of
 * the cells whose value is 0.  r2 then holds R2 and tie holds T of DESIGN.md 4.20 rule 2. */
#define ICV_RANK_MAX_CELLS (1 << 21)
int icv_rank_count(const icv_matrix *m, const int32_t *code, int32_t *stored, int32_t *flags, void *stream);
int icv_rank_scatter(const icv_matrix *m, const int32_t *code, int32_t w0, int32_t n_win, const int32_t *seg_off,
                     int32_t *cursor, uint64_t *keys, int32_t *payload, void *stream);
int icv_rank_sort(const uint64_t *keys, const int32_t *payload, int64_t n_entries, const int32_t *seg_off, int32_t n_win,
                  uint64_t *keys_sorted, int32_t *payload_sorted, void *stream);
int icv_rank_sums(const uint64_t *keys, const int32_t *payload, const int32_t *seg_off, int32_t w0, int32_t n_win,
                  int32_t longest, int32_t n_cols, int64_t n_pop, int32_t n_codes, int64_t *r2, int32_t *cnt, int64_t *tie,
                  int32_t *neg, void *stream);
int icv_rank_finish(const int32_t *stored, const int32_t *neg, const int32_t *cnt, const int64_t *n_cells, int64_t n_groups,
                    int32_t n_cols, int64_t n_pop, int64_t *r2, int64_t *tie, void *stream);

/* ---- tl.cnv_pool_neighbors: the exact mean of every row with the rows of its graph neighbours ------------
 * The graph is a device CSR structure of n vertices: g_indptr (device int64, n + 1, from 0, non-decreasing: trusted) and
 * g_indices (device int32, g_indptr[n] entries; never null, whatever the number of entries).  Its values are not an
 * argument: only the structure is read, and it need not be symmetric.  The neighbourhood of row i is
 * N(i) = {i} u {g_indices[e] : g_indptr[i] <= e < g_indptr[i + 1]}; an explicit diagonal entry does not count i twice, an
 * empty row gives {i}, a row may have any length.  Both entries enqueue on the stream and synchronise nothing.
 * icv_neighbor_pool_sizes: n_cells[i] (device int32, n) = L_i = |N(i)|.  *flags (device int32) is set to 0; then bit 1
 * (value 2) is set where a column lies outside [0, n) (it is not counted) and bit 2 (value 4) where the columns of a row
 * do not ascend strictly (a repeated column is counted twice: refuse such a graph).
 * icv_neighbor_pool: m as for icv_group_profiles (stored values are used as float64, an entry that is not stored is 0, a
 * stored 0.0 or -0.0 adds nothing; CSR columns need not be sorted but are unique within a row; a column outside
 * [0, n_cols) is passed over) with m->n_rows == n.  With q = rint(v 2^shift), ties to even, as int64, and S[i,w] the int64
 * sum of q over the rows of N(i): out[i * ldo + w] (device float64, n rows of ldo >= n_cols elements, 8-byte aligned) =
 * (double(S) / double(n_cells[i])) 2^-shift -- the conversion rounds to nearest even, the division is correctly rounded,
 * the scaling exact; S = 0 gives +0.0.  The caller chooses shift in [0, 40] so that 2^(10 + shift) max(L_i) stays below
 * 2^62 (min(40, 52 - bit_length(max L_i)) with every stored magnitude below 2^10) and passes the n_cells of
 * icv_neighbor_pool_sizes.  *flags is NOT reset: bit 0 (value 1) is set where a value that was read is not finite (it adds
 * nothing), bit 1 where a graph column lies outside [0, n) (skipped, never dereferenced).  Every output element is written
 * exactly once with plain stores; nothing of the size of the output is allocated.  n_cols has no limit.
 * Both return ICV_ERR_INVALID, before anything is launched, for a null pointer, n < 1 and, icv_neighbor_pool, n_cols < 1,
 * a shift outside [0, 40], ldo < n_cols, a format / dtype that does not exist, a dense ld < n_cols and m->n_rows != n. */
int icv_neighbor_pool_sizes(const int64_t *g_indptr, const int32_t *g_indices, int64_t n, int32_t *n_cells, int32_t *flags,
                            void *stream);
int icv_neighbor_pool(const icv_matrix *m, const int64_t *g_indptr, const int32_t *g_indices, int64_t n, int32_t shift,
                      const int32_t *n_cells, double *out, int64_t ldo, int32_t *flags, void *stream);

/* ---- tl.cnv_copy_states: multi-level copy-number calls of X_cnv by a K-state Viterbi chain ------------------
 * icv_copy_states_viterbi: rules 2-5 of the contract.  m and chr_start as for icv_states_viterbi.  levels (HOST pointer to
 * n_levels doubles, 2 <= n_levels <= 8, read before the call returns and passed to the kernel by value) holds the state
 * means: finite, strictly ascending, levels[neutral] == 0 (a -0.0 is used as 0.0), 0 <= neutral < n_levels.
 * h = 1 / (2 sigma^2) > 0, stay = log(1 - p) and sw = log(p / (n_levels - 1)) are the host's doubles, all finite.
 * states (device int8, n_rows x n_cols row-major, no padding) receives state - neutral, in
 * [-neutral, n_levels - 1 - neutral]; sign (the same layout) receives states clipped to -1 / 0 / +1, the format of
 * icv_states_viterbi; nonneutral[i] (device int32) the number of windows of row i that are not 0.  With the levels
 * (-a, 0, a) all three equal what icv_states_viterbi gives for the amplitude a, byte for byte.  One wavefront per row,
 * 10 bytes of LDS per window: 1 <= n_cols <= ICV_COPY_STATES_MAX_WINDOWS.  ICV_ERR_INVALID, with the rule in
 * icv_last_error and before anything is launched, for a null pointer, n_cols outside that range, n_chr outside
 * [1, n_cols], n_levels outside [2, 8], a neutral that is no index of a level or whose level is not 0, a level that is
 * not finite, levels that do not ascend strictly, an h that is not finite and > 0, a stay or sw that is not finite, and
 * an incomplete matrix.  No rows: ICV_OK, nothing is launched.  The result is a pure function of the arguments.  No
 * synchronisation. */
#define ICV_COPY_STATES_MAX_WINDOWS 16384
int icv_copy_states_viterbi(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, const double *levels,
                            int32_t n_levels, int32_t neutral, double h, double stay, double sw, int8_t *states,
                            int8_t *sign, int32_t *nonneutral, void *stream);

/* ---- tl.cnv_copy_posteriors and tl.cnv_copy_states_filter: posteriors of the model of tl.cnv_copy_states ---
 * icv_copy_posterior_chains: forward-backward along every chromosome of every row of m under the K-state model of
 * icv_copy_states_viterbi (m, chr_start, levels, n_levels = K, neutral and h as there); ps = 1 - p and
 * pw = p / (K - 1) are the host's doubles for a p in (0, 1), pw a normal float64.  The rules are those of
 * icv_posterior_chains with K states: b(s) = exp_(e_s - max e); pred(s) = (..((al(0) A(0,s)) + (al(1) A(1,s))) + ..) over
 * r ascending, u = pred b, c = (..(u(0) + u(1)) + ..), al = u / c; be_t(r) = (..((A(r,0) g(0)) + (A(r,1) g(1))) + ..) / c_{t+1}
 * with g = b_{t+1} be_{t+1}; the posterior is (al_t be_t) / (..(w(0) + w(1)) + ..).  Float64, no fused multiply-add, every
 * division correctly rounded: a pure function of the arguments, and with the levels (-a, 0, a) the bytes of
 * icv_posterior_chains for the amplitude a.  neutral_out (device float64, n_rows x n_cols row-major, no padding) receives
 * P(neutral); planes_out is null or receives all K planes (n_levels x n_rows x n_cols, plane s = P(state s)).  A window
 * that no chromosome covers gets 1.0 in the neutral plane and 0.0 in the others.  One wavefront per row, 8 (K + 1) bytes of
 * LDS per window: 1 <= n_cols <= ICV_COPY_POSTERIOR_MAX_WINDOWS(K).  ICV_ERR_INVALID, with the rule in icv_last_error and
 * before anything is launched or any pointer but levels is read, for a null m, chr_start, levels or neutral_out, n_cols
 * outside that range, n_chr outside [1, n_cols], every model that icv_copy_states_viterbi refuses, an h that is not finite
 * and > 0, a ps outside (0, 1), a pw that is not a normal float64 in (0, 1), and an incomplete matrix.  No rows: ICV_OK,
 * nothing is launched.  No synchronisation.
 * icv_copy_states_filter: icv_states_filter for calls that are levels.  states (device int8, values in [-7, 7]) and
 * p_neutral (device float64), both n_rows x n_cols row-major without padding.  A run is a maximal stretch of ONE level
 * other than 0 inside one chromosome (+1 +1 +2 +2 is two runs).  With q_t = int64(rint(p_neutral[i,t] 2^40)), a run [s, e)
 * is reset to 0 in filtered (device int8) iff double(sum of its q_t) / (double(e - s) 2^40) > max_p_normal (in [0, 1]);
 * every other window is copied.  sign (device int8) receives filtered clipped to -1 / 0 / +1, the format of
 * icv_states_viterbi.  nonneutral[i] / removed[i] (device int32) = the windows of filtered's row i that are not 0 / the
 * runs of row i that were reset.  *bad (device int32) is set to 0 and then to 1 where a call is outside [-7, 7] or a
 * posterior is not a number in [0, 1].  With calls in {-1, 0, +1} filtered, nonneutral, removed and bad are those of
 * icv_states_filter.  n_cols <= ICV_FILTER_MAX_WINDOWS (ICV_ERR_UNSUPPORTED beyond); ICV_ERR_INVALID for a null pointer,
 * n_rows < 0, n_cols < 1, n_chr outside [1, n_cols] or a max_p_normal outside [0, 1].  No synchronisation. */
#define ICV_COPY_POSTERIOR_LDS_BYTES 163840
#define ICV_COPY_POSTERIOR_MAX_WINDOWS(k) (ICV_COPY_POSTERIOR_LDS_BYTES / (8 * ((k) + 1)))
int icv_copy_posterior_chains(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, const double *levels,
                              int32_t n_levels, int32_t neutral, double h, double ps, double pw, double *neutral_out,
                              double *planes_out_or_null, void *stream);
int icv_copy_states_filter(const int8_t *states, const double *p_neutral, int64_t n_rows, int32_t n_cols,
                           const int32_t *chr_start, int32_t n_chr, double max_p_normal, int8_t *filtered, int8_t *sign,
                           int32_t *nonneutral, int32_t *removed, int32_t *bad, void *stream);

/* ---- tl.cnv_copy_states_fit: the E-step of the Baum-Welch fit of the model of tl.cnv_copy_states ------------
 * icv_copy_posterior_stats: forward-backward exactly as icv_copy_posterior_chains (the same arguments, rules and bits of
 * b, al_t, c_t, be_t, z_t and gamma_t), reduced per row to stats[i] = (N_0 .. N_{K-1}, M_0 .. M_{K-1}, S) (device float64,
 * n_rows x (2K + 1) row-major).  Per chromosome of T >= 1 windows the 2K + 1 sums start at 0.0 and take their terms for
 * t = T-1 down to 0: N_s += gamma_t(s); M_s += gamma_t(s) x_t (the product rounded before the add); for t <= T-2,
 * S += (st / c_{t+1}) / z_t with m(s) = (al_t(s) ps) g(s), g = b_{t+1} be_{t+1} and st = (..(m(0) + m(1)) + ..) + m(K-1).
 * The row's sums start at 0.0 and add the chromosome sums in ascending chromosome order; a chromosome without windows
 * and a window that no chromosome covers add nothing.  Float64, no fused multiply-add, no atomics: a pure function of the
 * arguments, and with the levels (-a, 0, a) S is the bytes of column 2 of icv_posterior_stats for the amplitude a.  One
 * wavefront per row; its LDS holds the row, K planes and 2K + 1 sums per chromosome:
 * ICV_COPY_POSTERIOR_STATS_LDS(n_cols, K, n_chr) <= ICV_COPY_POSTERIOR_LDS_BYTES, that is
 * 1 <= n_cols <= ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(K, n_chr).  ICV_ERR_INVALID, with the rule in icv_last_error, before
 * anything is launched or any pointer but levels is read and in the order of icv_copy_posterior_chains, for a null m,
 * chr_start, levels or stats, n_cols outside that range, n_chr outside [1, n_cols], every model and scalar that
 * icv_copy_posterior_chains refuses, and an incomplete matrix.  No rows: ICV_OK, nothing is launched.  No
 * synchronisation. */
#define ICV_COPY_POSTERIOR_STATS_LDS(n_cols, k, n_chr) (8 * (((k) + 1) * (n_cols) + (2 * (k) + 1) * (n_chr)))
#define ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(k, n_chr) \
    ((ICV_COPY_POSTERIOR_LDS_BYTES - 8 * (2 * (k) + 1) * (n_chr)) / (8 * ((k) + 1)))
int icv_copy_posterior_stats(const icv_matrix *m, const int32_t *chr_start, int32_t n_chr, const double *levels,
                             int32_t n_levels, int32_t neutral, double h, double ps, double pw, double *stats,
                             void *stream);

/* ---- tl.cnv_copy_segments: level-aware segment tables of the int8 levels of tl.cnv_copy_states ---------------
 * states (device int8, n_rows x n_cols row-major, no padding, any alignment) holds levels in [lo, hi], 0 neutral, with
 * -ICV_LEVEL_MAX <= lo <= 0 <= hi <= ICV_LEVEL_MAX; chr_start as for icv_segments_count.  A run is that of
 * icv_copy_states_filter: window t starts one iff states[i,t] != 0 and (t is a chromosome start or states[i,t-1] differs), it
 * ends one iff states[i,t] != 0 and (t + 1 == n_cols or t + 1 is a chromosome start or states[i,t+1] differs): +1 +1 +2 is
 * two runs.  Integer arithmetic: the results are a pure function of the arguments.
 * icv_level_segments_count / icv_level_segments_fill: icv_segments_count / icv_segments_fill for levels: *bad (device int32)
 * is set to 0 and then to 1 where a value lies outside [lo, hi]; seg_level (int8) is the byte of states at the run's start.
 * With lo = -1, hi = 1 they are the two three-state entries.  n_cols has no limit below int32.
 * icv_level_votes: rows and group_ptr as for icv_state_votes; counts (device int32, n_groups x (hi - lo + 1) x n_cols) is
 * zeroed and counts[g,p,w] receives the number of listed rows of group g with level lo + p at window w, the neutral plane
 * (p = -lo) included (integer atomic adds).  A row number outside [0, n_rows) is skipped; *bad as above, for the rows that
 * are listed.
 * icv_level_consensus: loss[g,w] / gain[g,w] (device int32, n_groups x n_cols) = the sums of the planes below / above the
 * neutral one.  The sign of consensus[g,w] (device int8) is that of icv_state_consensus on them (+ iff gain >= need[g] and
 * gain > loss, - iff loss >= need[g] and loss > gain, else 0), its magnitude the d in 1 .. hi (1 .. -lo) whose plane
 * sign d holds the largest count, the smallest such d on a tie.
 * icv_level_segments_support: for every segment of the consensus matrix (seg_row = the group) cells_min (int32) /
 * cells_sum (int64) = the minimum / the sum over its windows of loss or gain, by the sign of seg_level; level_min /
 * level_sum the same of the plane of seg_level.  A segment outside the tables, or with a level that is 0 or outside
 * [lo, hi], gets 0 in all four.
 * icv_segments_psum: for every segment k of the per-row tables (seg_row = the row of p_neutral, device float64 n_rows x
 * n_cols row-major without padding) psum[k] (device int64) = the sum over [seg_start, seg_end) of
 * q_t = int64(rint(p_neutral[i,t] 2^40)): double(psum) / (double(seg_end - seg_start) 2^40) is the mean of
 * icv_copy_states_filter, bit for bit.  *bad is set to 0 and then to 1 where a posterior INSIDE a segment is not a number
 * in [0, 1] (it adds 0).  Windows outside the segments are not read and are not validated.  A segment outside the plane
 * gets 0.  A run has no other limit than n_cols <= ICV_FILTER_MAX_WINDOWS, which keeps its sum inside int64
 * (ICV_ERR_UNSUPPORTED beyond).
 * All six: ICV_ERR_INVALID, with the rule in icv_last_error and before anything is launched, for a null pointer (the
 * tables of no segments and of no groups may be null), n_rows < 0 or another negative count, n_cols < 1, n_chr outside
 * [1, n_cols] and a level range that breaks -7 <= lo <= 0 <= hi <= 7.  No rows, no groups or no segments: ICV_OK, nothing
 * is launched.  No synchronisation. */
#define ICV_LEVEL_MAX 7
int icv_level_segments_count(const int8_t *states, int64_t n_rows, int32_t n_cols, const int32_t *chr_start, int32_t n_chr,
                             int32_t lo, int32_t hi, int64_t *counts, int32_t *bad, void *stream);
int icv_level_segments_fill(const int8_t *states, int64_t n_rows, int32_t n_cols, const int32_t *chr_start, int32_t n_chr,
                            const int64_t *offsets, int64_t n_segments, int64_t *seg_row, int32_t *seg_start,
                            int32_t *seg_end, int8_t *seg_level, void *stream);
int icv_level_votes(const int8_t *states, int64_t n_rows, int32_t n_cols, const int64_t *rows, int64_t n_listed,
                    const int64_t *group_ptr, int64_t n_groups, int32_t lo, int32_t hi, int32_t *counts, int32_t *bad,
                    void *stream);
int icv_level_consensus(const int32_t *counts, const int32_t *need, int64_t n_groups, int32_t n_cols, int32_t lo, int32_t hi,
                        int32_t *loss, int32_t *gain, int8_t *consensus, void *stream);
int icv_level_segments_support(const int64_t *seg_row, const int32_t *seg_start, const int32_t *seg_end,
                               const int8_t *seg_level, int64_t n_segments, const int32_t *counts, const int32_t *loss,
                               const int32_t *gain, int64_t n_groups, int32_t n_cols, int32_t lo, int32_t hi,
                               int32_t *cells_min, int64_t *cells_sum, int32_t *level_min, int64_t *level_sum, void *stream);
int icv_segments_psum(const double *p_neutral, int64_t n_rows, int32_t n_cols, const int64_t *seg_row,
                      const int32_t *seg_start, const int32_t *seg_end, int64_t n_segments, int64_t *psum, int32_t *bad,
                      void *stream);

/* ---- upload path of a mostly-zero DENSE host matrix (reference tl/_infercnv.py:115-116, :422-423: a dense adata.X of
 * log-counts is ~80 % zeros; PCIe is what a host-input call waits for) -- HOST functions (h_ pointers), no GPU needed:
 * icv_host_dense_row_nnz counts the stored entries (bit pattern != 0: NaN and -0.0 count) of every row of a row-major
 * float32 / float64 matrix on n_threads threads; the caller forms indptr (prefix sums, indptr[0] = 0);
 * icv_host_dense_pack writes the rows' column indices (int32, ascending) and values at indptr[r].  The arrays then cross
 * PCIe (8 or 12 bytes per stored entry instead of 4 or 8 per element) and icv_csr_scatter_dense (device pointers)
 * rebuilds the dense rows in HBM: out[r * ldo + c] = value, zeros elsewhere -- bit for bit the matrix a dense upload
 * would have delivered, so everything downstream is unchanged. */
int icv_host_dense_row_nnz(const void *h_x, int32_t dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                           int64_t *h_row_nnz, int32_t n_threads);
int icv_host_dense_pack(const void *h_x, int32_t dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                        const int64_t *h_indptr, int32_t *h_indices, void *h_values, int32_t n_threads);
/* The same in ONE pass over the input (what tl.infercnv uses: the host memory system is the bottleneck of the upload):
 * threads claim blocks of 16 rows in order, pack into their own staging area, take their place in the output through a
 * ticket handed on in block order and copy the block there; h_indptr (n_rows + 1) is written as well, *h_nnz = the
 * number of stored entries.  `capacity` = entries h_indices / h_values hold: ICV_ERR_NOMEM if the matrix has more
 * (h_indptr and *h_nnz are complete then; the entry arrays are not: call again with larger buffers). */
int icv_host_dense_pack_fused(const void *h_x, int32_t dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                              int64_t *h_indptr, int32_t *h_indices, void *h_values, int64_t capacity,
                              int32_t n_threads, int64_t *h_nnz);
int icv_csr_scatter_dense(const void *data, int32_t dtype, const int64_t *indptr, const int32_t *indices, int64_t n_rows,
                          int32_t n_cols, void *out, int64_t ldo, void *stream);

/* ---- misc --------------------------------------------------------------------------------- */
const char *icv_last_error(void);
int icv_version(void);
/* The developer knobs (environment variables ICV_FORCE_GENERIC, ICV_NO_X16, ICV_NO_SD, ICV_WARD_IN_PLACE,
 * ICV_WARD_COMPACT_X, ICV_PHASE_PROFILE: kernel routes / geometries for A/B timing and kernel-against-kernel tests) are
 * read once, at the first dispatch; a process that changes them afterwards calls this to have them read again. */
void icv_developer_knobs_reload(void);
/* number of visible HIP devices (0 without a GPU); never fails */
int icv_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* INFERCNV_HIP_H */
