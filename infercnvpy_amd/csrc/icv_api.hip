// C ABI (include/infercnv_hip.h) over the gfx950 kernels.  No torch types, no exceptions across
// the boundary; all data pointers are device pointers owned by the caller.
#include "../../include/infercnv_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <memory>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "icv_kernels.hpp"
#include "icv_kernel_ws.hpp"
#include "icv_kernel_x16.hpp"
#include "icv_kernel_se.hpp"
#include "icv_kernel_chain.hpp"
#include "icv_kernel_chainq.hpp"
#include "icv_kernel_pack.hpp"
#include "icv_kernel_util.hpp"
#include "icv_kernel_gene.hpp"
#include "icv_kernel_blocks.hpp"
#include "icv_corr.hpp"
#include "icv_pca.hpp"
#include "icv_knn.hpp"
#include "icv_graph.hpp"
#include "icv_leiden.hpp"
#include "icv_umap.hpp"
#include "icv_tsne.hpp"
#include "icv_states.hpp"
#include "icv_copy_states.hpp"
#include "icv_copy_posterior.hpp"
#include "icv_copy_hmmfit.hpp"
#include "icv_segments.hpp"
#include "icv_copy_segments.hpp"
#include "icv_hmmfit.hpp"
#include "icv_posterior.hpp"
#include "icv_pseudobulk.hpp"
#include "icv_profile_corr.hpp"
#include "icv_silhouette.hpp"
#include "icv_kmeans.hpp"
#include "icv_changepoint.hpp"
#include "icv_rank.hpp"
#include "icv_pool.hpp"
#include "icv_ward.hpp"
#include "icv_ward_strip.hpp"
#include "icv_plan.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ICV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorName(e_) + " (" + \
                                         hipGetErrorString(e_) + ")");                         \
    } while (0)

// One instantiation by an element-type code (ICV_F32 / ICV_F64, checked by the caller): f, a generic lambda, gets a value
// of the element type.  by_matrix adds std::true_type for a CSR matrix and std::false_type for a dense one.
template <typename F>
auto by_dtype(int32_t dtype, F&& f) {
    return dtype == ICV_F32 ? f(float{}) : f(double{});
}
template <typename F>
auto by_matrix(const icv_matrix* m, F&& f) {
    return by_dtype(m->dtype,
                    [&](auto t) { return m->format == ICV_CSR ? f(t, std::true_type{}) : f(t, std::false_type{}); });
}

// what every entry point that takes a matrix checks first: a row count, an element type and a format that exist
bool matrix_header_ok(const icv_matrix* m) {
    return m && m->n_rows >= 0 && (m->dtype == ICV_F32 || m->dtype == ICV_F64) &&
           (m->format == ICV_DENSE || m->format == ICV_CSR);
}
// the pointer its format cannot do without: the values of a dense matrix, the row offsets of a CSR one (a CSR without
// stored entries may come with null indices / values: they are never read then)
bool matrix_complete(const icv_matrix* m) { return m->format == ICV_DENSE ? m->values != nullptr : m->indptr != nullptr; }

// Developer knobs (environment variables that force a kernel route / geometry for A/B timing and for the tests that
// compare the kernels with each other).  They are read ONCE, at the first dispatch, not on every call (a
// getenv per dispatch, and a production call's route must not follow an environment edited under it); a test that
// changes them calls icv_developer_knobs_reload().
struct Knobs {
    bool force_generic, no_x16, no_x16_finite, no_sd, phase_profile, ward_in_place, no_mask_ring, no_fill_ring,
         no_chain_queues, no_gene_fused;
    int chain_far;         // ICV_CHAIN_FAR: entries a buffer offset may span in k_colchain_csrq (tests: a small value)
    int chain_pieces;      // ICV_CHAIN_PIECES: lanes per row of k_colchain_csrq (2 / 4 / 8 / 16; 0 = from the density)
    double ward_compact_x; // 0 = not set
    void load() {
        force_generic = std::getenv("ICV_FORCE_GENERIC") != nullptr;
        no_x16 = std::getenv("ICV_NO_X16") != nullptr;
        no_x16_finite = std::getenv("ICV_NO_X16_FINITE") != nullptr;  // k_smooth_x16 in its checked form only
        no_sd = std::getenv("ICV_NO_SD") != nullptr;
        phase_profile = std::getenv("ICV_PHASE_PROFILE") != nullptr;
        ward_in_place = std::getenv("ICV_WARD_IN_PLACE") != nullptr;
        no_mask_ring = std::getenv("ICV_NO_MASK_RING") != nullptr;
        no_fill_ring = std::getenv("ICV_NO_FILL_RING") != nullptr;
        no_chain_queues = std::getenv("ICV_NO_CHAIN_QUEUES") != nullptr;
        no_gene_fused = std::getenv("ICV_NO_GENE_FUSED") != nullptr;  // gene values through the three round-1 kernels
        const char* e = std::getenv("ICV_CHAIN_FAR");
        chain_far = e ? std::atoi(e) : 0;
        e = std::getenv("ICV_CHAIN_PIECES");
        chain_pieces = e ? std::atoi(e) : 0;
        e = std::getenv("ICV_WARD_COMPACT_X");
        ward_compact_x = e ? std::atof(e) : 0.0;
    }
};
std::mutex g_knobs_mu;
bool g_knobs_loaded = false;
Knobs g_knobs;
const Knobs& knobs() {
    std::lock_guard<std::mutex> lk(g_knobs_mu);
    if (!g_knobs_loaded) {
        g_knobs.load();
        g_knobs_loaded = true;
    }
    return g_knobs;
}

}  // namespace

struct icv_plan_s {
    icv::Plan p;
    std::mutex mu;
    std::atomic<bool> busy{false};  // a compute entry point is in its launch sequence (workspace in use)
    int device = -1;
    int n_cu = 0;
    int32_t *d_dst = nullptr, *d_src = nullptr, *d_wstart = nullptr, *d_wlen = nullptr;
    double* d_wdenom = nullptr;
    int32_t* d_pad = nullptr;
    int32_t* d_wpack = nullptr;
    unsigned* d_tie_n = nullptr;  // k_thr_mask_ring's tie counter + k_thr_mask_ties' done counter (zero between calls)
    int32_t *d_cov_col = nullptr, *d_cov_j0 = nullptr, *d_cov_cnt = nullptr;
    uint32_t* d_gv_pk = nullptr;  // k_gene_fused: per run, first window | #windows << 16
    int32_t* d_gv_mult = nullptr;   //               genes per run
    uint16_t* d_gv_col16 = nullptr;  //              input column -> run, or R (the kernel's NaN slot) where the gene has no value; padded to a multiple of 8 columns
    bool gv_fused_ok = false;
    int gv_mult_bytes = 2;  // bytes per run length in the kernel's LDS (1 where every run has at most 255 genes)
    int64_t* d_row_list = nullptr;  // cells handed back by k_smooth_ws to the generic kernel
    int* d_row_count = nullptr;
    int32_t* d_x16_form = nullptr;  // which form of k_smooth_x16 applied when a call launched both (1: FINITE)
    bool x16_both = false;          // the last compute call launched both forms
    int64_t row_list_cap = 0;
    // deferred profiling (icv_profile_begin / icv_profile_collect): event quadruples of the runs since begin
    bool prof_deferred = false;
    std::vector<hipEvent_t> prof_events;
    double* d_win_scratch = nullptr;  // Layout::win_global: per-workgroup window lines of k_smooth
    int64_t win_scratch_cap = 0;
    double* d_cell_part = nullptr;  // per-wavefront partial moments of the ws / x16 kernels
    int64_t cell_part_cap = 0;
    double* d_chunk_part = nullptr;  // k_smooth_x16<CHUNK>: per (chunk, workgroup, wavefront) moments
    int64_t chunk_part_cap = 0;      // in double2 elements
    double* d_hb_stats = nullptr;    // per-row moments when the caller passes no cell_stats (rows x 2)
    int64_t hb_stats_cap = 0;        // in rows
    uint16_t* d_dst16 = nullptr;
    uint32_t* d_x16_wdesc = nullptr;
    int32_t* d_blk_g0 = nullptr;  // per block: first-gene offset inside its chromosome (k_se_wtab)
    uint32_t *d_se_w0 = nullptr, *d_se_w1 = nullptr;   // k_smooth_se (plan: se_window_words)
    void* d_zrow = nullptr;  // CSR workspace: padded row, sized for float64
    size_t zrow_elems = 0;
    // Gene sets whose padded row does not fit LDS (float32: > ~40 000 genes, float64: > ~20 000): the
    // chromosomes are dealt into groups that do fit, each group is a plan of its own (windows only), and the
    // median / centring run on the float64 windows collected in HBM (smooth_split).
    std::vector<icv_plan_s*> parts;
    std::vector<int> part_woff;  // first window of every group in the full window list
    int parts_elem = 0;          // element size the groups were sized for (0: not built)
    int last_kernel = ICV_KERNEL_NONE;  // smoothing kernel of the last compute call (icv_plan_last_kernel)
    // the per-call workspace above is shared by all calls on this plan: a call on another stream than the previous
    // one first waits (on the device) for the previous call's work
    hipEvent_t done_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last = false;
};

namespace {

// grid of a kernel whose workgroups take the rows in turns: per_cu workgroups on every CU, at most one per row
int64_t cu_grid(const icv_plan_t pl, int per_cu, int64_t n_rows) {
    const int64_t grid = (int64_t)pl->n_cu * per_cu;
    return grid > n_rows ? n_rows : grid;
}

// plan-owned, grow-only device buffer: at least `need` elements of `elem_bytes` behind ptr.  After an allocation that
// failed the pointer is null and the capacity 0, so the next call allocates again.
template <typename T>
int grow(T*& ptr, int64_t& cap, int64_t need, size_t elem_bytes = sizeof(T)) {
    if (cap >= need) return ICV_OK;
    (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc((void**)&ptr, (size_t)need * elem_bytes));
    cap = need;
    return ICV_OK;
}

// thr == NULL: no threshold is applied and the chunk arguments are not looked at
bool chunk_args_ok(const void* thr, int64_t chunksize, int64_t row_phase) {
    return !thr || (chunksize >= 1 && row_phase >= 0 && row_phase < chunksize);
}

// one compute call at a time per plan (the plan owns the per-call workspace); released on scope exit
struct PlanBusy {
    icv_plan_t pl;
    bool ok;
    hipStream_t st = nullptr;
    bool entered = false;
    explicit PlanBusy(icv_plan_t p) : pl(p), ok(false) {
        bool expected = false;
        ok = p && p->busy.compare_exchange_strong(expected, true);
    }
    // Work of the previous call on this plan may still be in flight on ANOTHER stream and uses the same workspace
    // (row list, partial moments, zero row): this call's stream waits for it.  Same stream: already ordered.
    hipError_t enter(hipStream_t s) {
        st = s;
        entered = true;
        if (!pl->done_ev) {
            const hipError_t e = hipEventCreateWithFlags(&pl->done_ev, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        if (pl->has_last && pl->last_stream != s) return hipStreamWaitEvent(s, pl->done_ev, 0);
        return hipSuccess;
    }
    ~PlanBusy() {
        if (ok && entered && pl->done_ev) {
            if (hipEventRecord(pl->done_ev, st) == hipSuccess) {
                pl->last_stream = st;
                pl->has_last = true;
            }
        }
        if (ok) pl->busy.store(false);
    }
};
#define PLAN_BUSY_GUARD(pl)                                                                          \
    PlanBusy busy_guard_(pl);                                                                        \
    if (!busy_guard_.ok)                                                                             \
        return fail(ICV_ERR_INVALID, "plan busy: one compute call at a time per plan (see icv_plan_create)")
// after ensure_device: order this call behind the plan's previous call if that ran on another stream
#define PLAN_ENTER(stream_) HIP_TRY(busy_guard_.enter(static_cast<hipStream_t>(stream_)))

// stream-ordered temporary: freed on every exit path (error paths leaked their buffers)
struct AsyncBuf {
    void* p = nullptr;
    hipStream_t st = nullptr;
    ~AsyncBuf() {
        if (p) (void)hipFreeAsync(p, st);
    }
    hipError_t alloc(size_t bytes, hipStream_t s) {
        st = s;
        keep_pool();
        return hipMallocAsync(&p, bytes ? bytes : 16, s);
    }
    // The device's default memory pool gives everything back to the driver whenever the stream is synchronised (release
    // threshold 0), and the next temporary is a real allocation again: milliseconds of an idle GPU in front of a
    // 0.2 ms kernel for every caller that synchronises between calls.  Keep up to 6 GB of temporaries pooled (once
    // per device and process; the largest single temporary is the n x n correlation matrix of tl.ithcna: 2.5 GB at
    // 25 000 cells per group).
    static void keep_pool() {
        static std::atomic<unsigned long long> done{0};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return;
        const unsigned long long bit = 1ull << dev;
        if (done.fetch_or(bit) & bit) return;
        hipMemPool_t pool;
        if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
            uint64_t keep = 6ull << 30;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};
// events of a timed run: destroyed on exit unless handed over to the plan (deferred profiling)
struct EventSet {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool keep = false;
    ~EventSet() {
        if (!keep)
            for (auto& e : ev)
                if (e) (void)hipEventDestroy(e);
    }
};

int ensure_device(icv_plan_t pl) {
    std::lock_guard<std::mutex> lk(pl->mu);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (pl->device == dev) return ICV_OK;
    if (pl->device >= 0) return fail(ICV_ERR_INVALID, "plan is bound to another device");
    const icv::Plan& p = pl->p;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    pl->n_cu = prop.multiProcessorCount;
    auto up = [&](const void* h, size_t bytes, void** d) -> hipError_t {
        hipError_t e = hipMalloc(d, bytes ? bytes : 16);
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    HIP_TRY(up(p.dst.data(), p.dst.size() * 4 + 0, (void**)&pl->d_dst));
    HIP_TRY(up(p.src.data(), p.src.size() * 4, (void**)&pl->d_src));
    HIP_TRY(up(p.w_start.data(), p.w_start.size() * 4, (void**)&pl->d_wstart));
    HIP_TRY(up(p.w_len.data(), p.w_len.size() * 4, (void**)&pl->d_wlen));
    HIP_TRY(up(p.w_denom.data(), p.w_denom.size() * 8, (void**)&pl->d_wdenom));
    HIP_TRY(up(p.pad_idx.data(), p.pad_idx.size() * 4, (void**)&pl->d_pad));
    HIP_TRY(up(p.w_pack.data(), p.w_pack.size() * 4, (void**)&pl->d_wpack));
    {
        const unsigned zeros[2] = {0u, 0u};
        HIP_TRY(up(zeros, sizeof(zeros), (void**)&pl->d_tie_n));
        HIP_TRY(up(zeros, sizeof(int32_t), (void**)&pl->d_x16_form));
    }
    HIP_TRY(up(p.cov_col.data(), p.cov_col.size() * 4, (void**)&pl->d_cov_col));
    HIP_TRY(up(p.cov_j0.data(), p.cov_j0.size() * 4, (void**)&pl->d_cov_j0));
    HIP_TRY(up(p.cov_cnt.data(), p.cov_cnt.size() * 4, (void**)&pl->d_cov_cnt));
    {
        // tables of k_gene_fused (16-bit fields: the fused kernel applies where they fit)
        const size_t R = p.gv_run_j0.size();
        bool ok = p.W <= 65535 && R < 65535;
        std::vector<uint32_t> pk(R);
        for (size_t r = 0; r < R && ok; ++r) {
            ok = p.gv_run_cnt[r] <= 128 && p.gv_run_mult[r] <= 65535;  // (<= 128 windows per gene: gv_numpy_sum)
            pk[r] = (uint32_t)p.gv_run_j0[r] | ((uint32_t)p.gv_run_cnt[r] << 16);
        }
        std::vector<uint16_t> c16(((size_t)p.n_cols_all + 7) / 8 * 8, (uint16_t)R);
        for (int c = 0; c < p.n_cols_all && ok; ++c) c16[c] = p.gv_col_run[c] < 0 ? (uint16_t)R : (uint16_t)p.gv_col_run[c];
        pl->gv_fused_ok = ok;
        pl->gv_mult_bytes = 1;
        for (int32_t v : p.gv_run_mult)
            if (v > 255) pl->gv_mult_bytes = 2;
        HIP_TRY(up(pk.data(), pk.size() * 4, (void**)&pl->d_gv_pk));
        HIP_TRY(up(p.gv_run_mult.data(), p.gv_run_mult.size() * 4, (void**)&pl->d_gv_mult));
        HIP_TRY(up(c16.data(), c16.size() * 2, (void**)&pl->d_gv_col16));
    }
    HIP_TRY(up(p.dst16.data(), p.dst16.size() * 2, (void**)&pl->d_dst16));
    HIP_TRY(up(p.x16_wdesc.data(), p.x16_wdesc.size() * 4, (void**)&pl->d_x16_wdesc));
    HIP_TRY(up(p.blk_g0.data(), p.blk_g0.size() * 4, (void**)&pl->d_blk_g0));
    HIP_TRY(up(p.se_w0.data(), p.se_w0.size() * 4, (void**)&pl->d_se_w0));
    HIP_TRY(up(p.se_w1.data(), p.se_w1.size() * 4, (void**)&pl->d_se_w1));
    pl->zrow_elems = (size_t)icv::round_up(p.Gp, 4) + 4;  // >= Gp + 1: the trash slot reads 0
    HIP_TRY(hipMalloc(&pl->d_zrow, pl->zrow_elems * 8));
    pl->device = dev;
    return ICV_OK;
}

int check_matrix(const icv_plan_t pl, const icv_matrix* m) {
    if (!pl || !m) return fail(ICV_ERR_INVALID, "null plan or matrix");
    if (m->n_cols != pl->p.n_cols_all)
        return fail(ICV_ERR_INVALID, "matrix has " + std::to_string(m->n_cols) + " columns, plan expects " +
                                         std::to_string(pl->p.n_cols_all));
    if (m->dtype != ICV_F32 && m->dtype != ICV_F64) return fail(ICV_ERR_INVALID, "dtype must be ICV_F32 or ICV_F64");
    if (m->format != ICV_DENSE && m->format != ICV_CSR) return fail(ICV_ERR_INVALID, "format must be dense or csr");
    if (m->n_rows < 0) return fail(ICV_ERR_INVALID, "negative n_rows");
    if (m->n_rows > 0 && !m->values && !(m->format == ICV_CSR)) return fail(ICV_ERR_INVALID, "null values");
    if (m->format == ICV_DENSE && m->ld < m->n_cols) return fail(ICV_ERR_INVALID, "ld < n_cols");
    if (m->format == ICV_CSR && (!m->indptr || (!m->indices && m->values)))
        return fail(ICV_ERR_INVALID, "csr needs indptr and indices");
    return ICV_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Chromosome groups whose rows fit LDS at `elem_bytes` per gene (see icv_plan_s::parts).
int build_parts(icv_plan_t pl, int elem_bytes) {
    std::lock_guard<std::mutex> lk(pl->mu);
    if (pl->parts_elem >= elem_bytes) return ICV_OK;
    for (auto* q : pl->parts) icv_plan_destroy(q);
    pl->parts.clear();
    pl->part_woff.clear();
    pl->parts_elem = 0;
    const icv::Plan& p = pl->p;
    std::vector<int32_t> col_pos((size_t)p.n_cols_all, -1);
    {
        int rank = 0;
        for (int q = 0; q < p.Gp; ++q)
            if (p.src[q] >= 0) col_pos[p.src[q]] = rank++;
    }
    const int budget = (icv::kLdsLimit - icv::kScratchBytes - 64) / elem_bytes;  // padded genes per group
    int c0 = 0;
    while (c0 < p.n_chr) {
        int c1 = c0, genes = 0;
        while (c1 < p.n_chr) {
            const int g = p.chrom_off[c1 + 1] - p.chrom_off[c1];
            const int padded = (g + p.B - 1) / p.B * p.B;
            if (c1 > c0 && genes + padded > budget) break;
            genes += padded;
            ++c1;
        }
        const int lo = p.chrom_off[c0], hi = p.chrom_off[c1];
        std::vector<int32_t> cp((size_t)p.n_cols_all, -1), off((size_t)(c1 - c0 + 1));
        for (int g = 0; g < p.n_cols_all; ++g)
            if (col_pos[g] >= lo && col_pos[g] < hi) cp[g] = col_pos[g] - lo;
        for (int c = c0; c <= c1; ++c) off[c - c0] = p.chrom_off[c] - lo;
        icv_plan_s* part = new (std::nothrow) icv_plan_s();
        if (!part) return fail(ICV_ERR_NOMEM, "out of host memory");
        const std::string err =
            icv::build_plan(part->p, p.n_cols_all, cp.data(), c1 - c0, off.data(), p.window, p.step, p.B);
        if (!err.empty()) {
            delete part;
            return fail(ICV_ERR_INVALID, err);
        }
        const icv::Layout& pl_lay = elem_bytes == 4 ? part->p.lay32 : part->p.lay64;
        if (!pl_lay.fits) {
            icv_plan_destroy(part);
            for (auto* q : pl->parts) icv_plan_destroy(q);
            pl->parts.clear();
            pl->part_woff.clear();
            return fail(ICV_ERR_UNSUPPORTED,
                        "a single chromosome needs " + std::to_string(pl_lay.total) +
                            " bytes of LDS per workgroup (limit 163840): too many genes on one chromosome");
        }
        pl->parts.push_back(part);
        pl->part_woff.push_back(p.chr_pos[c0]);
        c0 = c1;
    }
    pl->parts_elem = elem_bytes;
    return ICV_OK;
}

int fill_params(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi, double lfc_clip,
                int32_t flags, float* out, int64_t ldo, double* cell_median, double* cell_stats, icv::KParams& K,
                const icv::Layout*& lay) {
    const icv::Plan& p = pl->p;
    if (!ref_lo) return fail(ICV_ERR_INVALID, "ref_lo is required");
    if (!(lfc_clip >= 0.0)) return fail(ICV_ERR_INVALID, "lfc_clip must be >= 0");
    if (!out || ldo < p.W) return fail(ICV_ERR_INVALID, "out is null or ldo < n_windows");
    lay = (m->dtype == ICV_F32) ? &p.lay32 : &p.lay64;
    if (!lay->fits) {  // chromosome-group fallback (smooth_split); fails if a single chromosome is too large
        const int rc = build_parts(pl, m->dtype == ICV_F32 ? 4 : 8);
        if (rc) return rc;
    }
    std::memset(&K, 0, sizeof(K));
    K.values = m->values;
    K.indptr = m->indptr;
    K.indices = m->indices;
    K.n_rows = m->n_rows;
    K.ld = m->ld;
    K.n_cols = m->n_cols;
    const int vn = (m->dtype == ICV_F32) ? 4 : 2;
    K.vec_ok = (m->format == ICV_DENSE) && aligned16(m->values) && aligned16(ref_lo) &&
               (!ref_hi || aligned16(ref_hi)) && (m->ld % vn == 0);
    K.ref_lo = ref_lo;
    K.ref_hi = ref_hi;
    K.zrow = pl->d_zrow;
    K.zrow_bytes = (int64_t)pl->zrow_elems * ((m->dtype == ICV_F32) ? 4 : 8);
    K.bounded = ref_hi != nullptr;
    K.trunc = flags & (ICV_FLAG_TRUNC_TO_INT | ICV_FLAG_ROUND_F32);
    K.cap = lfc_clip;
    K.dst = pl->d_dst;
    K.src = pl->d_src;
    K.w_start = pl->d_wstart;
    K.w_len = pl->d_wlen;
    K.w_denom = pl->d_wdenom;
    K.dst16 = pl->d_dst16;
    K.pad_idx = pl->d_pad;
    K.w_pack = pl->d_wpack;
    K.x16_wdesc = pl->d_x16_wdesc;
    K.blk_g0 = pl->d_blk_g0;
    K.x16_half = p.x16_half;
    K.n_pad = (int32_t)p.pad_idx.size();
    K.pyr_den = p.pyr_den;
    K.pyr_rcp = p.pyr_rcp;
    {
        const double capd = (m->dtype == ICV_F32) ? (double)(float)lfc_clip : lfc_clip;
        K.med_bound = capd * 1.000001 + 1e-30;
    }
    K.B = p.B;
    K.NB = p.NB;
    K.Gp = p.Gp;
    K.W = p.W;
    K.win_off = lay->win_off;
    K.scratch_off = lay->scratch_off;
    K.out = out;
    K.ldo = ldo;
    K.cell_median = cell_median;
    K.cell_stats = cell_stats;
    return ICV_OK;
}

typedef void (*SmoothKernel)(const icv::KParams);

// Which smoothing kernel a call takes and how it is launched.  pick_route decides it, ONCE per call; run_route carries
// it out, and the chunk thresholds take the count of partial-moment slots from it.
struct SmoothRoute {
    int kind = ICV_KERNEL_NONE;   // ICV_KERNEL_*
    SmoothKernel kern = nullptr;  // (ICV_KERNEL_SPLIT: none -- the chromosome groups take the generic kernel in turn)
    SmoothKernel kern_finite = nullptr;  // k_smooth_x16<FINITE>, launched in front of `kern` where K.fin_words is set
    int64_t grid = 0;
    int block = icv::NT, lds = 0;
    int64_t moment_slots = 0;     // per-chunk partial-moment slots the launch writes (grid x wavefronts); 0: per-cell moments
    bool writes_windows = false;  // the float64 windows (K.win_out) leave this launch
    int k0 = 0, k1 = 0;           // k_smooth_se: fraction bits of its bins
};

int run_kernel(const SmoothRoute& r, const icv::KParams& K, hipStream_t st) {
    const SmoothKernel kern = r.kern;
    const int64_t grid = r.grid;
    const int lds = r.lds, block = r.block;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (knobs().phase_profile) {
        // developer diagnostic: shader cycles per phase, summed over workgroups (thread 0 of each)
        unsigned long long* d = nullptr;
        HIP_TRY(hipMalloc((void**)&d, 32 * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(d, 0, 32 * sizeof(unsigned long long)));
        icv::KParams K2 = K;
        K2.dbg = d;
        K2.fin_words = nullptr;  // one launch: the checked form
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, st, K2);
        HIP_TRY(hipStreamSynchronize(st));
        unsigned long long h[32];
        HIP_TRY(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
        if (r.kind == ICV_KERNEL_X16) {  // k_smooth_x16 (-DICV_X_PROFILE): shader cycles per cell of wavefront 15
            (void)hipFree(d);
            std::fprintf(stderr, "[icv x16 profile] grid=%lld rows=%lld lds=%d cycles per cell: A: store %.0f, chains %.0f, S "
                                 "%.0f, barrier 1 %.0f, B: output+gather+clear %.0f, W %.0f, L %.0f, barrier 2 %.0f\n", (long long)grid,
                         (long long)K.n_rows, lds, (double)h[6] / (double)K.n_rows, (double)h[7] / (double)K.n_rows,
                         (double)h[0] / (double)K.n_rows, (double)h[1] / (double)K.n_rows,
                         (double)h[4] / (double)K.n_rows, (double)h[5] / (double)K.n_rows,
                         (double)h[2] / (double)K.n_rows, (double)h[3] / (double)K.n_rows);
            return ICV_OK;
        }
        (void)hipFree(d);
        if (r.kind == ICV_KERNEL_SD) {  // k_smooth_se (-DICV_SE_PROFILE=<thread>): work of phase 0..3, each followed by its barrier wait
            std::fprintf(stderr, "[icv se profile] grid=%lld rows=%lld cycles per cell of the profiled thread:", (long long)grid,
                         (long long)K.n_rows);
            const char* nm[8] = {"ph0", "A", "ph1", "B1", "ph2", "B2", "ph3", "B3"};
            for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %s %.0f", nm[i], (double)h[i] / (double)K.n_rows);
            std::fprintf(stderr, "\n");
            return ICV_OK;
        }
        const char* names[6] = {"L load+scatter", "S block sums", "W windows", "M2 rank/select", "O output",
                                "M1 pivot search"};
        double tot = 0;
        for (int i = 0; i < 6; ++i) tot += (double)h[i];
        std::fprintf(stderr, "[icv phase profile] grid=%lld rows=%lld lds=%d\n", (long long)grid,
                     (long long)K.n_rows, lds);
        for (int i = 0; i < 6; ++i)
            std::fprintf(stderr, "  %-16s %12.0f cycles/cell  %5.1f %%\n", names[i], (double)h[i] / (double)K.n_rows,
                         100.0 * (double)h[i] / tot);
        std::fprintf(stderr, "  [6] %.2f  [7] %.4f per cell (fast: median iterations, split cells; ws: phases are "
                             "A-wait, gather+L, B1-wait, S+emit, S01+B3, W+B4; [6] = selector scan cycles, [7] = fallback cells)\n",
                     (double)h[6] / (double)K.n_rows, (double)h[7] / (double)K.n_rows);
        return ICV_OK;
    }
    if (r.kern_finite) {
        // both forms back to back, no host synchronisation: each reads K.fin_words first and the one that does not
        // apply returns at once
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(r.kern_finite), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(r.kern_finite, dim3((unsigned)grid), dim3(block), lds, st, K);
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, st, K);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// plan-owned workspace of the kernels that hand cells back to the generic k_smooth: the list of those cells, its
// counter (zeroed here) and the per-wavefront partial moments
int hand_back_workspace(icv_plan_t pl, icv::KParams& K, hipStream_t st) {
    if (int rc = grow(pl->d_row_list, pl->row_list_cap, K.n_rows)) return rc;
    // 16 wavefront partial pairs per cell (k_smooth_x16; k_smooth_ws / k_smooth_se use the first 8)
    if (int rc = grow(pl->d_cell_part, pl->cell_part_cap, K.n_rows, 32 * sizeof(double))) return rc;
    K.cell_part = pl->d_cell_part;
    if (!pl->d_row_count) HIP_TRY(hipMalloc((void**)&pl->d_row_count, sizeof(int)));
    HIP_TRY(hipMemsetAsync(pl->d_row_count, 0, sizeof(int), st));
    K.row_list = pl->d_row_list;
    K.row_count = pl->d_row_count;
    return ICV_OK;
}

// cells a fast kernel handed back (more than 64 windows in the median bins, a stored NaN): the generic kernel
// recomputes them (it reads the device-side count and exits at once when the list is empty)
int launch_hand_back(icv_plan_t pl, const icv::KParams& K, hipStream_t st, bool csr) {
    const icv::Plan& p = pl->p;
    icv::KParams G = K;
    G.win_off = p.lay32.win_off;
    G.scratch_off = p.lay32.scratch_off;
    G.dbg = nullptr;
    const int need = (p.NB + icv::kThreads - 1) / icv::kThreads;
    void (*gk)(const icv::KParams);
    if (csr) gk = need <= 4 ? icv::k_smooth<float, true, 4> : icv::k_smooth<float, true, 8>;
    else gk = need <= 4 ? icv::k_smooth<float, false, 4> : icv::k_smooth<float, false, 8>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(gk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                p.lay32.total));
    hipLaunchKernelGGL(gk, dim3((unsigned)cu_grid(pl, 1, K.n_rows)), dim3(icv::NT), p.lay32.total, st, G);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// k_smooth_se: fraction bits of its bins.  A bin starts at 1.5 * 2^52 and must stay within 2^51 of it: at most B
// entries of |d| <= 2 cap each in S0 (units 2^-k0), sum of j |d| <= B (B - 1) / 2 * 2 cap in S1 (units 2^-k1).  Fewer
// than 40 bits (a clip value beyond ~100) and the input takes the kernels that build the row in LDS.
bool se_fraction_bits(const icv::Plan& p, double cap, int* k0, int* k1) {
    if (!p.se_ok || knobs().no_sd) return false;  // ICV_NO_SD: developer knob, the kernels with a row in LDS
    int e = 0;
    (void)std::frexp((double)p.B * 2.0 * cap + 1.0, &e);  // < 2^e
    const int a = 51 - e;
    (void)std::frexp((double)p.B * (double)(p.B - 1) * cap + 1.0, &e);
    const int b = 51 - e;
    if (a < 40 || b < 36) return false;
    *k0 = a;
    *k1 = b;
    return true;
}

// ---- the kernel instantiations of a plan's geometry (no decisions here: pick_route asks for them) ---------------------
// k_smooth_ws: float32 in block form, the row in LDS (dense, or rebuilt from the prepared CSR entries)
SmoothKernel ws_kernel(const icv::Plan& p, bool csr) {
    constexpr int U = icv::kFastUMax;
    const int need_b = (p.NB + icv::kThreads - 1) / icv::kThreads;
    const bool u10 = (p.B == 10 && p.window == 100);
    if (csr) {
        if (need_b <= 4) return u10 ? icv::k_smooth_ws<U, 4, 4, 10, 10, true> : icv::k_smooth_ws<U, 4, 4, 0, 0, true>;
        return (p.B == 5) ? icv::k_smooth_ws<U, 8, 4, 5, 0, true> : icv::k_smooth_ws<U, 8, 4, 0, 0, true>;
    }
    if (need_b <= 4) return u10 ? icv::k_smooth_ws<U, 4, 4, 10, 10, false> : icv::k_smooth_ws<U, 4, 4, 0, 0, false>;
    if (p.B == 5 && p.window == 250) return icv::k_smooth_ws<U, 8, 4, 5, 50, false>;
    return (p.B == 5) ? icv::k_smooth_ws<U, 8, 4, 5, 0, false> : icv::k_smooth_ws<U, 8, 4, 0, 0, false>;
}

// k_smooth_x16: window 100 / step 10 or window 250 / step 10 (the instantiations assume step 10: blocks between adjacent
// windows); null for every other geometry.  `win`: the float64 windows leave the kernel as well (chunk-moment mode only)
// FIN: the form without NaN handling, for a matrix whose reference means certify it finite (KParams::fin_words)
template <bool FIN>
SmoothKernel x16_kernel(const icv::Plan& p, bool chunk, bool win) {
    if (!p.x16_ok || p.step != 10) return nullptr;
    if (p.B == 10 && p.window == 100 && p.x16_fine == 4096)
        return win ? icv::k_smooth_x16<10, 10, 1, true, 4096, true, true, FIN>
                   : (chunk ? icv::k_smooth_x16<10, 10, 1, true, 4096, true, false, FIN>
                            : icv::k_smooth_x16<10, 10, 1, false, 4096, true, false, FIN>);
    if (p.B == 5 && p.window == 250 && p.x16_fine == 1024)
        return win ? icv::k_smooth_x16<5, 50, 2, true, 1024, false, true, FIN>
                   : (chunk ? icv::k_smooth_x16<5, 50, 2, true, 1024, false, false, FIN>
                            : icv::k_smooth_x16<5, 50, 2, false, 1024, false, false, FIN>);
    return nullptr;
}

// k_smooth_se.  Window registers per thread: 3 where the windows fit (<= 1 536: window 250 / step 10 at 20 000 genes has
// 1 472), else 4; entry slots per thread from the mean row length: PF x 512 slots should hold mean + 4 sigma (binomial)
// entries -- longer rows take the in-phase loop, any PF gives the same bits
SmoothKernel se_kernel(const icv::Plan& p, const icv_matrix* m, bool bounded, bool chunk, bool win) {
    const bool w3 = p.W <= 3 * icv::NT;
    if (win) {
        // calculate_gene_values: the float64 windows leave the kernel as well (four entry slots per thread whatever
        // the row length: any slot count gives the same bits, and this path is bound by the cells x genes output)
        if (w3) return bounded ? icv::k_smooth_se<3, true, true, 4, true> : icv::k_smooth_se<3, true, false, 4, true>;
        return bounded ? icv::k_smooth_se<4, true, true, 4, true> : icv::k_smooth_se<4, true, false, 4, true>;
    }
    if (!chunk) {
        if (w3) return bounded ? icv::k_smooth_se<3, false, true> : icv::k_smooth_se<3, false, false>;
        return bounded ? icv::k_smooth_se<4, false, true> : icv::k_smooth_se<4, false, false>;
    }
    int pf = 4;
    if (m->n_rows > 0) {
        double want = 0.0;
        if (m->_pad > 0) {
            want = (double)m->_pad;  // the caller's figure: the length most rows stay under (icv_matrix._pad)
        } else if (m->csr_end > m->csr_begin) {  // none: mean + 3.5 sigma of a binomial row length
            const double mean = (double)(m->csr_end - m->csr_begin) / (double)m->n_rows;
            const double dens = mean / (double)(m->n_cols > 0 ? m->n_cols : 1);
            want = mean + 3.5 * std::sqrt(mean * (dens < 1.0 ? 1.0 - dens : 0.0)) + 8.0;
        }
        if (want > 0.0) pf = want <= icv::NT ? 1 : want <= 2 * icv::NT ? 2 : want <= 3 * icv::NT ? 3 : 4;
    }
#define ICV_SE_PICK(MW, BD)                                                                              \
    (pf == 1 ? icv::k_smooth_se<MW, true, BD, 1> : pf == 2 ? icv::k_smooth_se<MW, true, BD, 2>           \
     : pf == 3 ? icv::k_smooth_se<MW, true, BD, 3> : icv::k_smooth_se<MW, true, BD, 4>)
    if (w3) return bounded ? ICV_SE_PICK(3, true) : ICV_SE_PICK(3, false);
    return bounded ? ICV_SE_PICK(4, true) : ICV_SE_PICK(4, false);
#undef ICV_SE_PICK
}

// the generic k_smooth on `lay` (the plan's own layout, or a chromosome group's): any dtype / format that fits LDS
template <typename T, bool CSR>
SmoothRoute generic_route(const icv_plan_t pl, const icv::Layout& lay, int64_t n_rows) {
    const icv::Plan& p = pl->p;
    SmoothRoute r;
    r.kind = ICV_KERNEL_GENERIC;
    const int need = (p.NB + icv::kThreads - 1) / icv::kThreads;
    r.kern = p.B <= 1 ? icv::k_smooth<T, CSR, 0> : (need <= 4 ? icv::k_smooth<T, CSR, 4> : icv::k_smooth<T, CSR, 8>);
    int per_cu = icv::kLdsLimit / lay.total;
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);  // 32 wavefronts per CU / 8 per workgroup
    r.grid = cu_grid(pl, per_cu, n_rows);
    r.lds = lay.total;
    r.writes_windows = true;
    return r;
}

// THE statement of which smoothing kernel a call takes, in the order of preference.  K: the call's parameters
// (fill_params; K.win_out set where the caller wants the float64 windows); want_chunk_moments: the caller asks for no
// per-cell moments, so a kernel that can forms them per chunk (moment_slots > 0 then: the caller owes it K.chunk_part).
//   1. a row that does not fit LDS: chromosome groups (smooth_split)
//   2. dense float32 in block form, 16-byte aligned: k_smooth_x16 where the geometry has an instantiation and there is
//      one reference row, else k_smooth_ws
//   3. CSR float32 with stored entries: k_smooth_se where its bins keep 40 fraction bits, else k_smooth_ws on prepared entries
//   4. everything else, float32 with an infinite clip value and the developer knob ICV_FORCE_GENERIC: k_smooth
// The float64 windows are written by k_smooth_x16 and k_smooth_se in chunk-moment mode only and never by k_smooth_ws:
// a call that wants them and cannot have them there takes k_smooth (ONE smoothing pass either way).
SmoothRoute pick_route(const icv_plan_t pl, const icv_matrix* m, const icv::KParams& K, const icv::Layout& lay,
                       bool want_chunk_moments) {
    const icv::Plan& p = pl->p;
    const Knobs& kn = knobs();
    SmoothRoute r;
    if (!lay.fits) {
        r.kind = ICV_KERNEL_SPLIT;
        r.writes_windows = true;
        return r;
    }
    const bool want_win = K.win_out != nullptr, csr = m->format == ICV_CSR;
    const bool fast_allowed = m->dtype == ICV_F32 && std::isfinite(K.cap) && !kn.force_generic;
    const bool win_ok = !want_win || want_chunk_moments;  // the x16 / se instantiations that write windows form chunk moments
    if (fast_allowed && !csr && p.ws_ok && K.vec_ok) {
        // ICV_NO_X16=1: developer knob, the previous generation
        const SmoothKernel xk = (K.bounded || kn.no_x16) ? nullptr : x16_kernel<false>(p, want_chunk_moments, want_win);
        if (xk && win_ok) {  // 16 wavefronts per cell, one 1024-thread workgroup per CU
            r.kind = ICV_KERNEL_X16;
            r.kern = xk;
            // ICV_NO_X16_FINITE=1: developer knob, the checked form whatever the means say
            if (K.fin_words && !kn.no_x16_finite) r.kern_finite = x16_kernel<true>(p, want_chunk_moments, want_win);
            r.grid = cu_grid(pl, 1, K.n_rows);
            r.block = icv::XT;
            r.lds = p.x16_lds;
            r.moment_slots = want_chunk_moments ? r.grid * icv::XWAVE : 0;
            r.writes_windows = want_win;
            return r;
        }
        if (!want_win) {
            r.kind = ICV_KERNEL_WS;
            r.kern = ws_kernel(p, false);
            r.lds = p.fast_lds;
            r.grid = cu_grid(pl, std::min(icv::kLdsLimit / r.lds, 4), K.n_rows);
            return r;
        }
    }
    if (fast_allowed && csr && m->csr_end > m->csr_begin) {
        if (se_fraction_bits(p, K.cap, &r.k0, &r.k1) && win_ok) {
            r.kind = ICV_KERNEL_SD;
            r.kern = se_kernel(p, m, K.bounded != 0, want_chunk_moments, want_win);
            r.lds = icv::kSeLds;
            r.grid = cu_grid(pl, icv::kLdsLimit / icv::kSeLds, K.n_rows);  // workgroups per CU from its LDS map
            r.moment_slots = want_chunk_moments ? r.grid * icv::NWAVE : 0;
            r.writes_windows = want_win;
            return r;
        }
        if (p.ws_ok && aligned16(K.ref_lo) && !want_win) {
            r.kind = ICV_KERNEL_WS_CSR;
            r.kern = ws_kernel(p, true);
            r.lds = p.fast_lds;
            r.grid = cu_grid(pl, std::min(icv::kLdsLimit / r.lds, 4), K.n_rows);
            return r;
        }
    }
    return by_matrix(m, [&](auto t, auto is_csr) {
        return generic_route<decltype(t), decltype(is_csr)::value>(pl, lay, K.n_rows);
    });
}

template <typename T>
void zero_row(icv_plan_t pl, const icv::KParams& K, hipStream_t st) {
    const int n = (int)pl->zrow_elems;
    hipLaunchKernelGGL(icv::k_zero_row<T>, dim3((n + 255) / 256), dim3(256), 0, st, K, static_cast<T*>(pl->d_zrow), n);
}

// ---- what a route's kernel needs before it starts (tmp: stream-ordered tables, released when the route has been issued)
// k_smooth_se (icv_kernel_se.hpp): the zero row, the per-column, per-window and per-block tables, the hand-back workspace
int prepare_se(icv_plan_t pl, const SmoothRoute& r, icv::KParams& K, hipStream_t st, AsyncBuf* tmp) {
    const icv::Plan& p = pl->p;
    AsyncBuf &tab = tmp[0], &hi = tmp[1], &wt = tmp[2], &g = tmp[3];
    zero_row<float>(pl, K, st);
    HIP_TRY(tab.alloc((size_t)K.n_cols * 16, st));
    HIP_TRY(wt.alloc((size_t)p.W * 16, st));
    HIP_TRY(g.alloc((size_t)(p.NB + 8) * 8, st));
    if (K.bounded) HIP_TRY(hi.alloc((size_t)K.n_cols * 4, st));
    K.sd_tab = tab.p;
    K.sd_tab_hi = K.bounded ? hi.as<float>() : nullptr;
    K.sd_wtab = wt.p;
    K.sd_g16 = g.as<double>();
    K.sd_scale = std::ldexp(1.0, r.k0);
    K.sd_qinv = std::ldexp(1.0, -r.k0);
    K.sd_q1inv = std::ldexp(1.0, -r.k1);
    K.sd_r = std::ldexp(1.0, r.k1 - r.k0);
    K.sd_window = p.window;
    hipLaunchKernelGGL(icv::k_se_table, dim3((unsigned)((K.n_cols + 255) / 256)), dim3(256), 0, st, K,
                       tab.as<icv::u32x4>(), const_cast<float*>(K.sd_tab_hi), (float)std::ldexp(1.0, r.k1));
    const int n_wt = p.W > p.NB + 8 ? p.W : p.NB + 8;
    hipLaunchKernelGGL(icv::k_se_wtab, dim3((unsigned)((n_wt + 255) / 256)), dim3(256), 0, st, K,
                       static_cast<const float*>(pl->d_zrow), pl->d_se_w0, pl->d_se_w1, wt.as<icv::u32x4>(),
                       g.as<double>(), K.sd_r);
    return hand_back_workspace(pl, K, st);
}

// k_smooth_ws / k_smooth_x16: the hand-back workspace; CSR input: the zero row and, on top of it, the prepared entries
// {LDS position, centred and clipped value} (k_csr_prepare)
int prepare_fast(icv_plan_t pl, const icv_matrix* m, icv::KParams& K, hipStream_t st, AsyncBuf* tmp) {
    const icv::Plan& p = pl->p;
    K.scratch_off = p.fast_scratch_off;
    if (m->format == ICV_CSR) {
        zero_row<float>(pl, K, st);
        const int64_t n = m->csr_end - m->csr_begin;
        int64_t g = (n + 255) / 256;
        if (g > 8192) g = 8192;
        HIP_TRY(tmp[0].alloc((size_t)(n > 0 ? n : 1) * 6, st));
        float* cv = tmp[0].as<float>();
        uint16_t* ps = reinterpret_cast<uint16_t*>(cv + (n > 0 ? n : 1));
        K.cvals = cv - m->csr_begin;  // indexed by the absolute entry number
        K.pos16 = ps - m->csr_begin;
        if (n > 0)
            hipLaunchKernelGGL(icv::k_csr_prepare, dim3((unsigned)g), dim3(256), 0, st, K, m->csr_begin, m->csr_end,
                               const_cast<uint16_t*>(K.pos16), const_cast<float*>(K.cvals));
    }
    K.hist_off = p.ws_hist_off;
    return hand_back_workspace(pl, K, st);
}

// k_smooth: the zero row of a CSR input; Layout::win_global: the per-workgroup window lines in HBM
int prepare_generic(icv_plan_t pl, const SmoothRoute& r, const icv_matrix* m, icv::KParams& K, const icv::Layout& lay,
                    hipStream_t st) {
    if (m->format == ICV_CSR) by_dtype(m->dtype, [&](auto t) { zero_row<decltype(t)>(pl, K, st); });
    if (lay.win_global) {
        if (int rc = grow(pl->d_win_scratch, pl->win_scratch_cap, r.grid * (int64_t)pl->p.W)) return rc;
        K.win_scratch = pl->d_win_scratch;
    }
    return ICV_OK;
}

int smooth_split(icv_plan_t pl, const icv_matrix* m, const icv::KParams& K, hipStream_t st);

// Carry a route out: the set-up of its kind, THE launch, the moment finish and the hand-back of the kernels that have
// them.  kernel_done (optional) is recorded right after the smoothing kernel itself, before those later launches, so
// that profiling reports the dominant kernel's own duration.  A call without rows launches nothing.
int run_route(icv_plan_t pl, const SmoothRoute& r, const icv_matrix* m, icv::KParams K, const icv::Layout& lay,
              hipStream_t st, hipEvent_t kernel_done = nullptr) {
    const icv::Plan& p = pl->p;
    if ((K.win_out && !r.writes_windows) || ((K.chunk_part != nullptr) != (r.moment_slots > 0)))
        return fail(ICV_ERR_INVALID, "the smoothing route and the call's parameters disagree");
    const bool hands_back = r.kind == ICV_KERNEL_WS || r.kind == ICV_KERNEL_WS_CSR || r.kind == ICV_KERNEL_X16 ||
                            r.kind == ICV_KERNEL_SD;
    AsyncBuf tmp[4];
    int rc = ICV_OK;
    if (r.kind == ICV_KERNEL_SPLIT) {
        if ((rc = smooth_split(pl, m, K, st))) return rc;
    } else if (r.grid >= 1) {
        if (r.kind == ICV_KERNEL_SD) rc = prepare_se(pl, r, K, st, tmp);
        else if (hands_back) rc = prepare_fast(pl, m, K, st, tmp);
        else rc = prepare_generic(pl, r, m, K, lay, st);
        if (rc) return rc;
        icv::KParams L = K;  // (K itself goes on to the hand-back launch)
        if (r.kind == ICV_KERNEL_X16) {
            L.win_off = p.x16_s01_off;
            L.hist_off = p.x16_hist_off;
            L.scratch_off = p.x16_scratch_off;
            if (r.kern_finite) {
                L.x16_form = pl->d_x16_form;
            } else {
                L.fin_words = nullptr;  // one launch, the checked form
            }
        }
        if ((rc = run_kernel(r, L, st))) return rc;
    }
    if (kernel_done) HIP_TRY(hipEventRecord(kernel_done, st));
    if (hands_back && r.grid >= 1) {
        // per-wavefront partial moments -> cell_stats (cells handed back are overwritten by k_smooth below); in
        // chunk-moment mode the kernel has reduced them per chunk itself
        const dim3 fg((unsigned)((K.n_rows + 255) / 256));
        if (!K.chunk_part && r.kind == ICV_KERNEL_X16)
            hipLaunchKernelGGL(icv::k_stats_finish_n, fg, dim3(256), 0, st, K.cell_part, K.n_rows, icv::XWAVE, K.cell_stats);
        else if (!K.chunk_part)
            hipLaunchKernelGGL(icv::k_stats_finish, fg, dim3(256), 0, st, K.cell_part, K.n_rows, K.cell_stats);
        if ((rc = launch_hand_back(pl, K, st, m->format == ICV_CSR))) return rc;
    }
    pl->last_kernel = r.kind;
    pl->x16_both = r.kern_finite != nullptr && r.grid >= 1 && !knobs().phase_profile;  // (the profile run launches one form)
    return ICV_OK;
}

// float64 windows of all cells, chromosome group by chromosome group (every pass re-reads the rows and keeps only
// its group's genes), into win[n_rows x W].  K: parameters of the full plan (fill_params).
int split_windows(icv_plan_t pl, const icv_matrix* m, const icv::KParams& K, double* win, hipStream_t st) {
    const bool f32 = m->dtype == ICV_F32;
    for (size_t k = 0; k < pl->parts.size(); ++k) {
        icv_plan_t part = pl->parts[k];
        int rc = ensure_device(part);
        if (rc) return rc;
        const icv::Plan& q = part->p;
        const icv::Layout& lay = f32 ? q.lay32 : q.lay64;
        icv::KParams P = K;
        P.dst = part->d_dst;
        P.src = part->d_src;
        P.w_start = part->d_wstart;
        P.w_len = part->d_wlen;
        P.w_denom = part->d_wdenom;
        P.dst16 = part->d_dst16;
        P.pad_idx = part->d_pad;
        P.w_pack = part->d_wpack;
        P.n_pad = (int32_t)q.pad_idx.size();
        P.B = q.B;
        P.NB = q.NB;
        P.Gp = q.Gp;
        P.W = q.W;
        P.win_off = lay.win_off;
        P.scratch_off = lay.scratch_off;
        P.zrow = part->d_zrow;
        P.zrow_bytes = (int64_t)part->zrow_elems * (f32 ? 4 : 8);
        P.win_out = win + pl->part_woff[k];
        P.win_ld = pl->p.W;
        P.win_only = 1;
        P.row_list = nullptr;
        P.row_count = nullptr;
        // (the generic kernel whatever the group's geometry: the median and the centring run on the collected windows)
        const SmoothRoute r = by_matrix(m, [&](auto t, auto csr) {
            return generic_route<decltype(t), decltype(csr)::value>(part, lay, P.n_rows);
        });
        if ((rc = run_route(part, r, m, P, lay, st))) return rc;
    }
    return ICV_OK;
}

// steps 1-4 for a gene set whose row does not fit LDS: windows by chromosome group, then median and centring
// on the float64 windows in HBM
int smooth_split(icv_plan_t pl, const icv_matrix* m, const icv::KParams& K, hipStream_t st) {
    const int64_t n = K.n_rows;
    if (n < 1) return ICV_OK;
    const int W = pl->p.W;
    AsyncBuf win_b, med_b;
    // (a caller that wants the float64 windows -- calculate_gene_values -- with a contiguous buffer gets them here)
    const bool own = !(K.win_out && K.win_ld == W);
    if (own) HIP_TRY(win_b.alloc((size_t)n * W * sizeof(double), st));
    HIP_TRY(med_b.alloc((size_t)n * sizeof(double), st));
    double *win = own ? win_b.as<double>() : K.win_out, *med = med_b.as<double>();
    int rc = split_windows(pl, m, K, win, st);
    if (!rc && own && K.win_out)
        HIP_TRY(hipMemcpy2DAsync(K.win_out, (size_t)K.win_ld * sizeof(double), win, (size_t)W * sizeof(double),
                                 (size_t)W * sizeof(double), (size_t)n, hipMemcpyDeviceToDevice, st));
    if (!rc) {
        hipLaunchKernelGGL(icv::k_row_median, dim3((unsigned)n), dim3(256), 0, st, win, n, W, med);
        hipLaunchKernelGGL(icv::k_win_finish, dim3((unsigned)n), dim3(256), 0, st, win, n, W, med, K.out, K.ldo,
                           K.cell_median, K.cell_stats);
        if (hipGetLastError() != hipSuccess) rc = fail(ICV_ERR_HIP, "split smoothing launch failed");
    }
    return rc;
}

int launch_apply(const icv_matrix* m, const icv::KParams& K, const double* thr, int64_t chunksize,
                 int64_t row_phase, hipStream_t st) {
    if (K.n_rows < 1) return ICV_OK;
    by_matrix(m, [&](auto t, auto csr) {
        hipLaunchKernelGGL((icv::k_apply_thr<decltype(t), decltype(csr)::value>), dim3((unsigned)K.n_rows), dim3(256), 0, st,
                           K, thr, chunksize, row_phase);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // namespace

// ---- reference profile in the reference's evaluation order (csrc/icv_kernel_chain.hpp) ------------------------------
namespace {
int current_cu_count() {  // (hipGetDeviceProperties costs a fraction of a millisecond: asked once per device)
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return 256;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    hipDeviceProp_t prop;
    n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

// line -> tile of ChainLaunch's split (tile t owns the lines [t * n_lines / grid, (t + 1) * n_lines / grid))
__global__ void k_chain_line_tiles(int n_lines, int grid, uint16_t* line_tile) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= grid) return;
    const int l0 = (int)((int64_t)t * n_lines / grid), l1 = (int)((int64_t)(t + 1) * n_lines / grid);
    for (int l = l0; l < l1; ++l) line_tile[l] = (uint16_t)t;
}

static_assert(icv::kFinWords == ICV_FINITE_WORDS, "the words the header promises");
// icv::kFinWords workgroups take the columns in turns.  words (optional): words[workgroup] = 1 if one of the means
// the workgroup wrote is NaN or infinite, else 0 -- written unconditionally, so the buffer needs no clearing.  A chain
// s = fl(s + x_r) that met a NaN stays NaN and one that met an infinity stays infinite (or turns NaN at the opposite
// one), so all-zero words over the chains of ALL rows of a matrix say that every element of it is finite.
template <typename T>
__global__ void __launch_bounds__(1024) k_chain_mean(const T* acc, int n, T denom, T* out, uint32_t* words) {
    int bad = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const T q = acc[i] / denom;  // IEEE division (numpy: true_divide(sum, n) in the matrix dtype)
        out[i] = q;
        bad |= !__builtin_isfinite(q);
    }
    if (!words) return;  // (uniform)
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) words[blockIdx.x] = bad ? 1u : 0u;
}

template <typename T>
int colchain_dense(const icv_matrix* m, const int32_t* rows, int64_t n_sel, T* acc, hipStream_t st) {
    const icv::ChainLaunch L(m->n_cols, (int)sizeof(T), current_cu_count());
    constexpr int EPL = 16 / (int)sizeof(T);
    // the buffer's last row goes through the guarded tail when a 16-byte segment load could run past the end; with a
    // row list the kernel itself looks whether the list ends with that row (one scalar load: nothing is read back)
    int64_t tail = -1, n_dma = n_sel;
    if ((int64_t)(m->_pad > 0 ? m->_pad : 0) + (int64_t)(m->n_cols + EPL - 1) / EPL * EPL > m->ld) {
        tail = m->n_rows - 1;
        if (!rows) n_dma = n_sel - 1;
    }
    typedef void (*kern_t)(const T*, int64_t, int, int, int, const int32_t*, int64_t, int64_t, T*);
    const kern_t kern = rows ? (kern_t)icv::k_colchain<T, true> : (kern_t)icv::k_colchain<T, false>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                icv::kChLdsFull));
    hipLaunchKernelGGL(kern, dim3(L.dense_grid), dim3(icv::kChThreads), L.lds_bytes, st, (const T*)m->values, m->ld,
                       m->n_cols, L.n_units, L.lds_bytes, rows, n_dma, tail, acc);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

template <typename T>
int colchain_csr(const icv_matrix* m, const int32_t* rows, int64_t n_sel, double scale, T* acc, hipStream_t st) {
    const icv::ChainLaunch L(m->n_cols, (int)sizeof(T), current_cu_count());
    if (L.grid > 65535) return fail(ICV_ERR_UNSUPPORTED, "icv_colchain: more than 65535 column tiles");
    AsyncBuf lt_b, bounds_b;
    HIP_TRY(lt_b.alloc((size_t)L.n_lines * sizeof(uint16_t), st));
    const int esz_shift_q = sizeof(T) == 4 ? 2 : 3;
    const size_t tab_lds = (size_t)icv::kQTabRows * (size_t)((L.grid + 2) | 1) * sizeof(uint16_t) +
                           (size_t)L.n_lines * sizeof(uint16_t);
    if (m->n_cols <= 65535 && tab_lds <= 160 * 1024 && !knobs().no_chain_queues) {
        // per-column queues (csrc/icv_kernel_chainq.hpp): 16-bit tile-major bounds table + the streamed chain
        hipLaunchKernelGGL(k_chain_line_tiles, dim3((L.grid + 255) / 256), dim3(256), 0, st, L.n_lines, L.grid,
                           lt_b.as<uint16_t>());
        const int64_t n_tb = (n_sel + icv::kQTabRows - 1) / icv::kQTabRows;
        HIP_TRY(bounds_b.alloc((size_t)n_tb * (L.grid + 1) * icv::kQTabRows * sizeof(uint16_t), st));
        typedef void (*tb_t)(const int64_t*, const int32_t*, const int32_t*, int64_t, const uint16_t*, int, int, int,
                             uint32_t*);
        const tb_t tb = rows ? (tb_t)icv::k_csr_tile_bounds16<true> : (tb_t)icv::k_csr_tile_bounds16<false>;
        if (tab_lds > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tb), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)tab_lds));
        hipLaunchKernelGGL(tb, dim3((unsigned)n_tb), dim3(256), tab_lds, st, m->indptr, m->indices, rows, n_sel,
                           lt_b.as<uint16_t>(), L.n_lines, esz_shift_q, L.grid, bounds_b.as<uint32_t>());
        typedef void (*kq_t)(const T*, const int64_t*, const int32_t*, int64_t, const int32_t*, int64_t, int, int, int,
                             const uint16_t*, T, int, T*);
        // lanes per row (= entry slots / 4) from the mean number of entries a row has in the WIDEST tile (from the
        // caller's row-length hint, icv_matrix._pad: the length most rows stay under, where there is one).  Measured on
        // 500 000 x 20 000 (profiles/r06_csr_means_density.txt): 16 slots up to ~8 entries per row and tile (beyond, too
        // many rounds hold a row past the slots, whose guarded loads wait behind the loads in flight), 32 slots to ~28.
        // Rows beyond the slots take the guarded loads: any choice gives the same bits.
        int pieces = 4;
        {
            const double rows_all = m->n_rows > 0 ? (double)m->n_rows : 1.0;
            double per_row = (double)(m->csr_end - m->csr_begin) / rows_all;
            if (m->_pad > 0 && (double)m->_pad > per_row) per_row = (double)m->_pad;
            const int tile_lines = (L.n_lines + L.grid - 1) / L.grid;
            const double mu = per_row * (double)(tile_lines * (128 / (int)sizeof(T))) / (double)(m->n_cols > 0 ? m->n_cols : 1);
            pieces = mu <= 2.0 ? 2 : mu <= 8.5 ? 4 : mu <= 28.0 ? 8 : 16;
            const int forced = knobs().chain_pieces;
            if (forced == 2 || forced == 4 || forced == 8 || forced == 16) pieces = forced;
        }
#define ICV_KQ(P) (rows ? (kq_t)icv::k_colchain_csrq<T, true, P> : (kq_t)icv::k_colchain_csrq<T, false, P>)
        const kq_t kq = pieces == 2 ? ICV_KQ(2) : pieces == 4 ? ICV_KQ(4) : pieces == 8 ? ICV_KQ(8) : ICV_KQ(16);
#undef ICV_KQ
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kq), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    icv::kChLdsFull));
        // (always the whole LDS of a CU: the ring of LDS rows is the work in flight; with more tiles than CUs the
        // workgroups take the CUs in turns)
        hipLaunchKernelGGL(kq, dim3(L.grid), dim3(icv::kChThreads), icv::kChLdsFull, st, (const T*)m->values, m->indptr,
                           m->indices, m->n_rows, rows, n_sel, m->n_cols, L.n_lines, icv::kChLdsFull,
                           (const uint16_t*)bounds_b.as<uint16_t>(), (T)scale,
                           knobs().chain_far > 0 ? knobs().chain_far : icv::kQFar, acc);
        HIP_TRY(hipGetLastError());
        return ICV_OK;
    }
    const int64_t n_blk = (n_sel + icv::kCcBlock - 1) / icv::kCcBlock;
    HIP_TRY(bounds_b.alloc((size_t)n_blk * (L.grid + 1) * icv::kCcBlock * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_chain_line_tiles, dim3((L.grid + 255) / 256), dim3(256), 0, st, L.n_lines, L.grid,
                       lt_b.as<uint16_t>());
    const int esz_shift = sizeof(T) == 4 ? 2 : 3;
    if (rows)
        hipLaunchKernelGGL(icv::k_csr_tile_bounds<true>, dim3((unsigned)n_blk), dim3(256), 0, st, m->indptr, m->indices,
                           rows, n_sel, lt_b.as<uint16_t>(), esz_shift, L.grid, bounds_b.as<uint32_t>());
    else
        hipLaunchKernelGGL(icv::k_csr_tile_bounds<false>, dim3((unsigned)n_blk), dim3(256), 0, st, m->indptr, m->indices,
                           rows, n_sel, lt_b.as<uint16_t>(), esz_shift, L.grid, bounds_b.as<uint32_t>());
    typedef void (*kern_t)(const T*, const int64_t*, const int32_t*, int64_t, const int32_t*, int64_t, int, int, int,
                           const uint32_t*, T, T*);
    const kern_t kern = rows ? (kern_t)icv::k_colchain_csr<T, true> : (kern_t)icv::k_colchain_csr<T, false>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                icv::kChLdsFull));
    hipLaunchKernelGGL(kern, dim3(L.grid), dim3(icv::kChThreads), L.lds_bytes, st, (const T*)m->values, m->indptr,
                       m->indices, m->n_rows, rows, n_sel, m->n_cols, L.n_lines, L.lds_bytes,
                       (const uint32_t*)bounds_b.as<uint32_t>(), (T)scale, acc);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}
}  // namespace


extern "C" {

const char* icv_last_error(void) { return g_err.c_str(); }
int icv_version(void) { return 101; }

void icv_developer_knobs_reload(void) {
    std::lock_guard<std::mutex> lk(g_knobs_mu);
    g_knobs.load();
    g_knobs_loaded = true;
}

int icv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int icv_plan_create(int32_t n_cols_all, const int32_t* h_col_pos, int32_t n_chr, const int32_t* h_chrom_offsets,
                    int32_t window, int32_t step, icv_plan_t* out) {
    if (!h_col_pos || !h_chrom_offsets || !out) return fail(ICV_ERR_INVALID, "null argument");
    icv_plan_s* pl = new (std::nothrow) icv_plan_s();
    if (!pl) return fail(ICV_ERR_NOMEM, "out of host memory");
    std::string err;
    try {
        err = icv::build_plan(pl->p, n_cols_all, h_col_pos, n_chr, h_chrom_offsets, window, step);
    } catch (const std::bad_alloc&) {
        delete pl;
        return fail(ICV_ERR_NOMEM, "out of host memory");
    }
    if (!err.empty()) {
        delete pl;
        return fail(ICV_ERR_INVALID, err);
    }
    *out = pl;
    return ICV_OK;
}

void icv_plan_destroy(icv_plan_t pl) {
    if (!pl) return;
    for (auto* q : pl->parts) icv_plan_destroy(q);
    pl->parts.clear();
    if (pl->device >= 0) {
        (void)hipFree(pl->d_dst);
        (void)hipFree(pl->d_src);
        (void)hipFree(pl->d_wstart);
        (void)hipFree(pl->d_wlen);
        (void)hipFree(pl->d_wdenom);
        (void)hipFree(pl->d_pad);
        (void)hipFree(pl->d_wpack);
        (void)hipFree(pl->d_tie_n);
        (void)hipFree(pl->d_cov_col);
        (void)hipFree(pl->d_cov_j0);
        (void)hipFree(pl->d_cov_cnt);
        (void)hipFree(pl->d_gv_pk);
        (void)hipFree(pl->d_gv_mult);
        (void)hipFree(pl->d_gv_col16);
        (void)hipFree(pl->d_row_list);
        (void)hipFree(pl->d_row_count);
        (void)hipFree(pl->d_x16_form);
        (void)hipFree(pl->d_cell_part);
        (void)hipFree(pl->d_chunk_part);
        (void)hipFree(pl->d_hb_stats);
        (void)hipFree(pl->d_win_scratch);
        (void)hipFree(pl->d_dst16);
        (void)hipFree(pl->d_x16_wdesc);
        (void)hipFree(pl->d_blk_g0);
        (void)hipFree(pl->d_se_w0);
        (void)hipFree(pl->d_se_w1);
        (void)hipFree(pl->d_zrow);
        if (pl->done_ev) (void)hipEventDestroy(pl->done_ev);
    }
    delete pl;
}

int icv_plan_get_info(icv_plan_t pl, icv_plan_info* info) {
    if (!pl || !info) return fail(ICV_ERR_INVALID, "null argument");
    const icv::Plan& p = pl->p;
    info->n_cols_all = p.n_cols_all;
    info->n_genes_used = p.n_used;
    info->n_chr = p.n_chr;
    info->window = p.window;
    info->step = p.step;
    info->n_windows = p.W;
    info->block = p.B;
    info->n_blocks = p.NB;
    info->padded_len = p.Gp;
    info->lds_bytes_f32 = p.lay32.total;
    info->lds_bytes_f64 = p.lay64.total;
    int per_cu = p.lay32.fits ? icv::kLdsLimit / p.lay32.total : 0;
    info->workgroups_per_cu_f32 = per_cu > 4 ? 4 : per_cu;
    return ICV_OK;
}

int icv_plan_last_route(icv_plan_t pl, int32_t* kind) {
    if (!pl || !kind) return fail(ICV_ERR_INVALID, "null argument");
    *kind = pl->last_kernel;
    return ICV_OK;
}

int icv_plan_last_kernel(icv_plan_t pl, int32_t* kind) {
    if (!pl || !kind) return fail(ICV_ERR_INVALID, "null argument");
    *kind = pl->last_kernel;
    if (pl->last_kernel == ICV_KERNEL_X16 && pl->x16_both && pl->d_x16_form) {
        // both forms were launched and the device chose: the form that applied left its mark (waits for that call)
        if (pl->has_last) HIP_TRY(hipStreamSynchronize(pl->last_stream));
        int32_t form = 0;
        HIP_TRY(hipMemcpy(&form, pl->d_x16_form, sizeof(form), hipMemcpyDeviceToHost));
        if (form) *kind = ICV_KERNEL_X16_FINITE;
    }
    return ICV_OK;
}

int icv_plan_last_handed_back(icv_plan_t pl, int64_t* n) {
    if (!pl || !n) return fail(ICV_ERR_INVALID, "null argument");
    *n = 0;
    const int k = pl->last_kernel;
    const bool hands_back = k == ICV_KERNEL_WS || k == ICV_KERNEL_WS_CSR || k == ICV_KERNEL_X16 || k == ICV_KERNEL_SD;
    if (!hands_back || !pl->d_row_count) return ICV_OK;  // (k_smooth and the split path rank every cell themselves)
    int count = 0;
    HIP_TRY(hipMemcpy(&count, pl->d_row_count, sizeof(int), hipMemcpyDeviceToHost));
    *n = count;
    return ICV_OK;
}

int icv_plan_chr_pos(icv_plan_t pl, int32_t* h_chr_pos) {
    if (!pl || !h_chr_pos) return fail(ICV_ERR_INVALID, "null argument");
    std::memcpy(h_chr_pos, pl->p.chr_pos.data(), pl->p.chr_pos.size() * sizeof(int32_t));
    return ICV_OK;
}

int icv_plan_window_table(icv_plan_t pl, int32_t* h_start, int32_t* h_len) {
    if (!pl || !h_start || !h_len) return fail(ICV_ERR_INVALID, "null argument");
    std::memcpy(h_start, pl->p.w_start_sorted.data(), pl->p.W * sizeof(int32_t));
    std::memcpy(h_len, pl->p.w_len_sorted.data(), pl->p.W * sizeof(int32_t));
    return ICV_OK;
}

int icv_plan_se_tables(icv_plan_t pl, int32_t* h_applies, int32_t* h_col_block, int32_t* h_col_offset,
                       int32_t* h_block_gene0, uint32_t* h_w0, uint32_t* h_w1) {
    if (!pl || !h_applies) return fail(ICV_ERR_INVALID, "null argument");
    const icv::Plan& p = pl->p;
    *h_applies = p.se_ok ? 1 : 0;
    if (!p.se_ok) return ICV_OK;
    if (h_col_block && h_col_offset)
        for (int g = 0; g < p.n_cols_all; ++g) {
            const int pos = p.dst[g];
            h_col_block[g] = pos < 0 ? -1 : pos / p.B;
            h_col_offset[g] = pos < 0 ? 0 : pos % p.B;
        }
    if (h_block_gene0) std::memcpy(h_block_gene0, p.blk_g0.data(), (size_t)p.NB * sizeof(int32_t));
    if (h_w0) std::memcpy(h_w0, p.se_w0.data(), (size_t)p.W * sizeof(uint32_t));
    if (h_w1) std::memcpy(h_w1, p.se_w1.data(), (size_t)p.W * sizeof(uint32_t));
    return ICV_OK;
}

int icv_plan_gene_runs(icv_plan_t pl, int32_t* h_n_runs, int32_t* h_run_first, int32_t* h_run_count,
                       int32_t* h_run_genes, int32_t* h_col_run) {
    if (!pl || !h_n_runs) return fail(ICV_ERR_INVALID, "null argument");
    const icv::Plan& p = pl->p;
    const size_t R = p.gv_run_j0.size();
    *h_n_runs = (int32_t)R;
    if (h_run_first) std::memcpy(h_run_first, p.gv_run_j0.data(), R * sizeof(int32_t));
    if (h_run_count) std::memcpy(h_run_count, p.gv_run_cnt.data(), R * sizeof(int32_t));
    if (h_run_genes) std::memcpy(h_run_genes, p.gv_run_mult.data(), R * sizeof(int32_t));
    if (h_col_run) std::memcpy(h_col_run, p.gv_col_run.data(), (size_t)p.n_cols_all * sizeof(int32_t));
    return ICV_OK;
}

int icv_colsum(const icv_matrix* m, const int32_t* row_group, int32_t n_groups, double* sums, void* stream) {
    if (!m || !sums || n_groups < 1) return fail(ICV_ERR_INVALID, "bad colsum arguments");
    if (m->n_rows == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nc = m->n_cols;
    if (m->format == ICV_CSR) {
        // one 1024-thread workgroup per (slab, column tile), the whole LDS of a CU each: two slabs per CU
        const int n_cu = current_cu_count();
        int rows_per_slab = (int)((m->n_rows + (int64_t)n_cu * 2 - 1) / ((int64_t)n_cu * 2));
        if (rows_per_slab < 64) rows_per_slab = 64;
        const int64_t n_slabs = (m->n_rows + rows_per_slab - 1) / rows_per_slab;
        const int n_tiles = (nc + icv::kCsrTileCols - 1) / icv::kCsrTileCols;
        const int lds = (nc < icv::kCsrTileCols ? nc : icv::kCsrTileCols) * (int)sizeof(double);
        AsyncBuf partial_b;
        HIP_TRY(partial_b.alloc((size_t)n_slabs * nc * sizeof(double), st));
        double* partial = partial_b.as<double>();
        dim3 grid((unsigned)n_tiles, (unsigned)n_slabs), block(icv::kCsThreads);
        return by_dtype(m->dtype, [&](auto t) {
            using T = decltype(t);
            const auto kern = row_group ? icv::k_colsum_csr<T, true> : icv::k_colsum_csr<T, false>;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            for (int g = 0; g < n_groups; ++g) {
                hipLaunchKernelGGL(kern, grid, block, lds, st, (const T*)m->values, m->indptr, m->indices, m->n_rows, nc,
                                   row_group, g, rows_per_slab, partial);
                hipLaunchKernelGGL(icv::k_colsum_finish, dim3((nc + 63) / 64), dim3(1024), 0, st, partial, (int)n_slabs, nc,
                                   sums + (int64_t)g * nc);
            }
            HIP_TRY(hipGetLastError());
            return (int)ICV_OK;
        });
    }
    // slab height from the row count alone (the sums must not depend on the device): 1024 rows stream fastest
    // (tools/microbench_colsum.hip), shorter slabs keep every CU busy on small matrices
    const int rows_per_slab = m->n_rows >= 65536 ? 1024 : 256;
    const int64_t n_slabs = (m->n_rows + rows_per_slab - 1) / rows_per_slab;
    AsyncBuf partial_b;
    HIP_TRY(partial_b.alloc((size_t)n_slabs * nc * sizeof(double), st));
    double* partial = partial_b.as<double>();
    dim3 grid((nc + 255) / 256, (unsigned)n_slabs), block(256);
    for (int g = 0; g < n_groups; ++g) {
        by_dtype(m->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(icv::k_colsum_dense<T>, grid, block, 0, st, (const T*)m->values, m->n_rows, m->ld, nc,
                               row_group, g, rows_per_slab, partial);
        });
        hipLaunchKernelGGL(icv::k_colsum_finish, dim3((nc + 63) / 64), dim3(1024), 0, st, partial, (int)n_slabs, nc,
                           sums + (int64_t)g * nc);
    }
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- the reference-order float32 chain by blocks (csrc/icv_kernel_blocks.hpp): row shards that do not take turns -----
namespace {
struct BlocksLayout {  // one workspace, laid out here (the caller allocates icv_colchain_blocks_workspace() bytes)
    int64_t n_slabs, n_blocks;
    size_t partial_off, start_off, slab_rec_off, rec_off, count_off, stash_off, bytes;
    unsigned stash_cap;
    BlocksLayout(int64_t n_rows, int32_t n_cols) {
        n_slabs = (n_rows + icv::kBkSlab - 1) / icv::kBkSlab;
        if (n_slabs < 1) n_slabs = 1;
        n_blocks = n_slabs * icv::kBkPerSlab;
        const size_t nc = (size_t)(n_cols > 0 ? n_cols : 1);
        auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        partial_off = 0;
        start_off = up(partial_off + (size_t)n_slabs * nc * 8);
        slab_rec_off = up(start_off + (size_t)n_slabs * nc * 8);
        rec_off = up(slab_rec_off + (size_t)n_slabs * nc * 4);
        count_off = up(rec_off + (size_t)n_blocks * nc * 4);
        stash_off = up(count_off + 256);
        // stash: the blocks that cannot be summarised -- 0.1-1 % of the (block, column) pairs of a shard that starts
        // inside the chains, ~1 % + the first few thousand rows of a shard that starts them; 3 % here, the rest is
        // replayed from the matrix
        const size_t want = (size_t)n_blocks * nc / 32 + 4096;
        stash_cap = (unsigned)(want < 0x7ffffff0u ? want : 0x7ffffff0u);
        bytes = up(stash_off + (size_t)stash_cap * icv::kBkRows * 4);
    }
};
int blocks_check(const icv_matrix* m, const void* ws) {
    if (!m || !ws) return fail(ICV_ERR_INVALID, "null matrix or workspace");
    if (m->format != ICV_DENSE || m->dtype != ICV_F32)
        return fail(ICV_ERR_UNSUPPORTED, "the block form of the chain takes dense float32 matrices (others: icv_colchain)");
    if (m->n_rows < 0 || m->n_cols < 1 || m->ld < m->n_cols) return fail(ICV_ERR_INVALID, "bad matrix");
    return ICV_OK;
}
}  // namespace

int icv_colchain_blocks_workspace(int64_t n_rows, int32_t n_cols, int64_t* bytes) {
    if (!bytes || n_rows < 0 || n_cols < 1) return fail(ICV_ERR_INVALID, "bad colchain_blocks_workspace arguments");
    *bytes = (int64_t)BlocksLayout(n_rows, n_cols).bytes;
    return ICV_OK;
}

int icv_colchain_blocks_sums(const icv_matrix* m, void* workspace, double* total, void* stream) {
    int rc = blocks_check(m, workspace);
    if (rc) return rc;
    if (!total) return fail(ICV_ERR_INVALID, "total is required");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BlocksLayout L(m->n_rows, m->n_cols);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + L.partial_off);
    HIP_TRY(hipMemsetAsync(total, 0, (size_t)m->n_cols * sizeof(double), st));
    if (m->n_rows == 0) return ICV_OK;
    dim3 grid((m->n_cols + 255) / 256, (unsigned)L.n_slabs);
    hipLaunchKernelGGL(icv::k_colsum_dense<float>, grid, dim3(256), 0, st, (const float*)m->values, m->n_rows, m->ld,
                       m->n_cols, (const int32_t*)nullptr, 0, icv::kBkSlab, partial);
    hipLaunchKernelGGL(icv::k_colsum_finish, dim3((m->n_cols + 63) / 64), dim3(1024), 0, st, partial, (int)L.n_slabs,
                       m->n_cols, total);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_colchain_blocks_records(const icv_matrix* m, void* workspace, const double* est_start, void* stream) {
    int rc = blocks_check(m, workspace);
    if (rc) return rc;
    if (m->n_rows == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BlocksLayout L(m->n_rows, m->n_cols);
    char* w = static_cast<char*>(workspace);
    const double* partial = reinterpret_cast<const double*>(w + L.partial_off);
    double* slab_start = reinterpret_cast<double*>(w + L.start_off);
    HIP_TRY(hipMemsetAsync(w + L.count_off, 0, 256, st));
    hipLaunchKernelGGL(icv::k_blocks_prefix, dim3((m->n_cols + 255) / 256), dim3(256), 0, st, partial, (int)L.n_slabs,
                       m->n_cols, est_start, slab_start);
    dim3 grid((m->n_cols + 255) / 256, (unsigned)L.n_slabs);
    hipLaunchKernelGGL(icv::k_chain_records, grid, dim3(256), 0, st, (const float*)m->values, m->n_rows, m->ld, m->n_cols,
                       slab_start, reinterpret_cast<uint32_t*>(w + L.rec_off), reinterpret_cast<uint32_t*>(w + L.slab_rec_off),
                       reinterpret_cast<float*>(w + L.stash_off), reinterpret_cast<unsigned*>(w + L.count_off), L.stash_cap);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_colchain_blocks_scan(const icv_matrix* m, void* workspace, float* acc, int32_t col0, int32_t col1,
                             uint64_t* d_replayed, void* stream) {
    int rc = blocks_check(m, workspace);
    if (rc) return rc;
    if (!acc || col0 < 0 || col1 > m->n_cols || col0 > col1) return fail(ICV_ERR_INVALID, "bad colchain_blocks_scan arguments");
    if (m->n_rows == 0 || col1 == col0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BlocksLayout L(m->n_rows, m->n_cols);
    char* w = static_cast<char*>(workspace);
    // (the column range: ranks pipeline the scan over column groups, as the chained form does)
    const int nc = col1 - col0;
    // one wavefront per column, four per workgroup, up to eight workgroups per CU at a time
    int64_t grid = ((int64_t)nc + 3) / 4;
    const int64_t cap = (int64_t)current_cu_count() * 8;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(icv::k_chain_scan, dim3((unsigned)grid), dim3(256), 0, st,
                       (const float*)m->values + col0, m->n_rows, m->ld, nc, (int64_t)m->n_cols,
                       reinterpret_cast<const uint32_t*>(w + L.rec_off) + col0,
                       reinterpret_cast<const uint32_t*>(w + L.slab_rec_off) + col0,
                       reinterpret_cast<const float*>(w + L.stash_off), acc + col0,
                       reinterpret_cast<unsigned long long*>(d_replayed));
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_colchain(const icv_matrix* m, const int32_t* rows, int64_t n_sel, double scale, void* acc, void* stream) {
    if (!m || !acc) return fail(ICV_ERR_INVALID, "bad colchain arguments");
    if (m->dtype != ICV_F32 && m->dtype != ICV_F64) return fail(ICV_ERR_INVALID, "dtype must be ICV_F32 or ICV_F64");
    if (!rows) n_sel = m->n_rows;
    if (n_sel < 0 || n_sel > m->n_rows) return fail(ICV_ERR_INVALID, "icv_colchain: n_sel out of range");
    if (n_sel == 0 || m->n_cols == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m->format != ICV_DENSE && m->format != ICV_CSR) return fail(ICV_ERR_INVALID, "format must be dense or csr");
    return by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        if constexpr (decltype(csr)::value) return colchain_csr<T>(m, rows, n_sel, scale, (T*)acc, st);
        else return colchain_dense<T>(m, rows, n_sel, (T*)acc, st);
    });
}

int icv_colchain_mean(const void* acc, int32_t dtype, int32_t n_cols, int64_t count, void* mean, void* stream) {
    return icv_colchain_mean_finite(acc, dtype, n_cols, count, mean, nullptr, stream);
}

int icv_colchain_mean_finite(const void* acc, int32_t dtype, int32_t n_cols, int64_t count, void* mean,
                             uint32_t* finite_words, void* stream) {
    if (!acc || !mean || count < 1 || n_cols < 0) return fail(ICV_ERR_INVALID, "bad colchain_mean arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype != ICV_F32 && dtype != ICV_F64) return fail(ICV_ERR_INVALID, "dtype must be ICV_F32 or ICV_F64");
    if (finite_words && (reinterpret_cast<uintptr_t>(finite_words) & 15))
        return fail(ICV_ERR_INVALID, "icv_colchain_mean_finite: finite_words must be 16-byte aligned");
    if (n_cols == 0 && !finite_words) return ICV_OK;  // (no column: every word 0)
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_chain_mean<T>, dim3(icv::kFinWords), dim3(1024), 0, st, (const T*)acc, n_cols, (T)count,
                           (T*)mean, finite_words);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_colmean_csc(const void* values, int32_t dtype, const int64_t* colptr, const int32_t* row_idx, int32_t n_cols,
                    const int32_t* row_group, int32_t group, double scale, void* mean, void* stream) {
    if (!values || !colptr || !row_idx || !mean || n_cols < 0) return fail(ICV_ERR_INVALID, "bad colmean_csc arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_cols == 0) return ICV_OK;
    if (dtype != ICV_F32 && dtype != ICV_F64) return fail(ICV_ERR_INVALID, "dtype must be ICV_F32 or ICV_F64");
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_colpair_csc<T>, dim3((n_cols + 63) / 64), dim3(64), 0, st, (const T*)values, colptr,
                           row_idx, n_cols, row_group, group, (T)scale, (T*)mean);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_colsum_pairwise(const void* xt, int32_t dtype, int64_t n_rows, int32_t n_cols, int64_t ld, void* sums,
                        void* stream) {
    if (!xt || !sums || n_rows < 0 || n_cols < 0 || ld < n_rows) return fail(ICV_ERR_INVALID, "bad colsum_pairwise arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_cols == 0) return ICV_OK;
    if (dtype != ICV_F32 && dtype != ICV_F64) return fail(ICV_ERR_INVALID, "dtype must be ICV_F32 or ICV_F64");
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_colpair_dense<T>, dim3((n_cols + 63) / 64), dim3(64), 0, st, (const T*)xt, n_rows, n_cols,
                           ld, (T*)sums);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_infercnv_smooth(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi,
                        double lfc_clip, int32_t flags, float* out, int64_t ldo, double* cell_median,
                        double* cell_stats, void* stream) {
    int rc = check_matrix(pl, m);
    if (rc) return rc;
    PLAN_BUSY_GUARD(pl);
    if (!cell_median || !cell_stats) return fail(ICV_ERR_INVALID, "cell_median and cell_stats are required");
    if ((rc = ensure_device(pl))) return rc;
    PLAN_ENTER(stream);
    icv::KParams K;
    const icv::Layout* lay;
    if ((rc = fill_params(pl, m, ref_lo, ref_hi, lfc_clip, flags, out, ldo, cell_median, cell_stats, K, lay)))
        return rc;
    return run_route(pl, pick_route(pl, m, K, *lay, false), m, K, *lay, static_cast<hipStream_t>(stream));
}

int icv_chunk_thresholds(const double* cell_stats, int64_t n_rows, int64_t chunksize, int64_t row_phase,
                         int32_t n_windows, double dynamic_threshold, double* thr, void* stream) {
    if (!cell_stats || !thr || !chunk_args_ok(thr, chunksize, row_phase))
        return fail(ICV_ERR_INVALID, "bad chunk threshold arguments");
    if (n_rows < 1) return ICV_OK;
    const int64_t n_chunks = (n_rows + row_phase + chunksize - 1) / chunksize;
    hipLaunchKernelGGL(icv::k_chunk_thr, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       cell_stats, n_rows, chunksize, row_phase, n_windows, dynamic_threshold, thr);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_apply_threshold(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi,
                        double lfc_clip, int32_t flags, float* out, int64_t ldo, const double* cell_median,
                        const double* thr, int64_t chunksize, int64_t row_phase, void* stream) {
    int rc = check_matrix(pl, m);
    if (rc) return rc;
    PLAN_BUSY_GUARD(pl);
    if (!cell_median || !thr || chunksize < 1) return fail(ICV_ERR_INVALID, "bad apply_threshold arguments");
    if ((rc = ensure_device(pl))) return rc;
    PLAN_ENTER(stream);
    icv::KParams K;
    const icv::Layout* lay;
    if ((rc = fill_params(pl, m, ref_lo, ref_hi, lfc_clip, flags, out, ldo, const_cast<double*>(cell_median),
                          nullptr, K, lay)))
        return rc;
    return launch_apply(m, K, thr, chunksize, row_phase, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {
// the stage times of a run from its four events (waits for the last one)
int read_profile(const hipEvent_t* ev, icv_profile* prof) {
    HIP_TRY(hipEventSynchronize(ev[3]));
    HIP_TRY(hipEventElapsedTime(&prof->smooth_ms, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&prof->thresholds_ms, ev[1], ev[2]));
    HIP_TRY(hipEventElapsedTime(&prof->apply_ms, ev[2], ev[3]));
    HIP_TRY(hipEventElapsedTime(&prof->total_ms, ev[0], ev[3]));
    return ICV_OK;
}

// steps 1-5 of the chunk kernel (icv_infercnv_run); win_out != nullptr: the float64 windows before centring as well
// (icv_infercnv_run_windows).  The caller holds the plan (PLAN_BUSY_GUARD + PLAN_ENTER).
int run_steps(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi, double lfc_clip,
              double dynamic_threshold, int64_t chunksize, int64_t row_phase, int32_t flags, float* out, int64_t ldo,
              double* cell_median, double* cell_stats, double* thr, icv_profile* prof, double* win_out, int64_t ldw,
              const uint32_t* finite_words, void* stream) {
    int rc;
    const bool do_thr = !std::isnan(dynamic_threshold);
    hipStream_t st = static_cast<hipStream_t>(stream);
    icv::KParams K;
    const icv::Layout* lay;
    if ((rc = fill_params(pl, m, ref_lo, ref_hi, lfc_clip, flags, out, ldo, cell_median, cell_stats, K, lay)))
        return rc;
    K.win_out = win_out;
    K.win_ld = ldw;
    K.fin_words = finite_words;
    // cell_stats == NULL: the caller only wants the thresholds.  The per-row moments then live in a plan-owned
    // buffer, and where k_smooth_x16 runs they are not formed per cell at all: the kernel accumulates them per
    // chunk (one wavefront reduction per chunk instead of per cell).
    int64_t n_chunks = 1, cs_eff = m->n_rows > 0 ? m->n_rows : 1, ph_eff = 0;
    if (do_thr) {
        cs_eff = chunksize;
        ph_eff = row_phase;
        n_chunks = (m->n_rows + row_phase + chunksize - 1) / chunksize;
        if (n_chunks < 1) n_chunks = 1;
    }
    // chunk moments are asked for as long as the partial slots of all chunks stay within 64 MB (slots per chunk: the
    // larger of k_smooth_x16's n_cu workgroups x 16 wavefronts and k_smooth_se's full grid x 8 wavefronts)
    const int64_t se_slots = ((int64_t)pl->n_cu * (icv::kLdsLimit / icv::kSeLds)) * icv::NWAVE;
    const int64_t x16_slots = (int64_t)pl->n_cu * icv::XWAVE;
    const int64_t n_part = se_slots > x16_slots ? se_slots : x16_slots;
    const bool lean = !cell_stats && m->n_rows > 0;
    const SmoothRoute route = pick_route(pl, m, K, *lay, lean && n_chunks * n_part <= (int64_t)(64 << 20) / 16);
    const int64_t n_slots = route.moment_slots;  // of the launch: slots of absent workgroups do not exist
    const bool chunk_mode = n_slots > 0;
    if (lean) {
        if ((rc = grow(pl->d_hb_stats, pl->hb_stats_cap, m->n_rows, 2 * sizeof(double)))) return rc;
        K.cell_stats = pl->d_hb_stats;
    }
    if (chunk_mode) {
        if ((rc = grow(pl->d_chunk_part, pl->chunk_part_cap, n_chunks * n_slots, 2 * sizeof(double)))) return rc;
        HIP_TRY(hipMemsetAsync(pl->d_chunk_part, 0, (size_t)(n_chunks * n_slots) * 2 * sizeof(double), st));
        HIP_TRY(hipMemsetAsync(pl->d_hb_stats, 0, (size_t)m->n_rows * 2 * sizeof(double), st));
        K.chunk_part = pl->d_chunk_part;
        K.chunksize = cs_eff;
        K.row_phase = ph_eff;
    }
    EventSet evs;
    hipEvent_t* ev = evs.ev;
    const bool deferred = !prof && pl->prof_deferred;
    const bool timed = prof || deferred;
    if (timed) {
        for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[0], st));
    }
    if ((rc = run_route(pl, route, m, K, *lay, st, timed ? ev[1] : nullptr))) return rc;
    if (do_thr && chunk_mode) {
        hipLaunchKernelGGL(icv::k_chunk_thr_part, dim3((unsigned)n_chunks), dim3(256), 0, st, pl->d_chunk_part,
                           (int)n_slots, pl->d_hb_stats, m->n_rows, chunksize, row_phase, pl->p.W,
                           dynamic_threshold, thr);
        HIP_TRY(hipGetLastError());
    } else if (do_thr && m->n_rows > 0) {
        rc = icv_chunk_thresholds(K.cell_stats, m->n_rows, chunksize, row_phase, pl->p.W, dynamic_threshold, thr,
                                  stream);
        if (rc) return rc;
    }
    if (timed) HIP_TRY(hipEventRecord(ev[2], st));
    if (do_thr && !(flags & ICV_FLAG_NO_APPLY) && (rc = launch_apply(m, K, thr, chunksize, row_phase, st))) return rc;
    if (timed) HIP_TRY(hipEventRecord(ev[3], st));
    if (deferred) {  // no synchronisation here: the times are read by icv_profile_collect
        for (int i = 0; i < 4; ++i) pl->prof_events.push_back(ev[i]);
        evs.keep = true;
    } else if (prof) {
        return read_profile(ev, prof);
    }
    return ICV_OK;
}

// gene values of n rows from their float64 windows: the fused kernel where a cell's windows and run values fit LDS,
// the three round-1 kernels on a cells x n_cov temporary otherwise
int gene_from_windows(icv_plan_t pl, const double* win, int64_t ldw, int64_t n, const double* thr, int64_t chunksize,
                      int64_t row_phase, double* gene_out, int64_t ldg, hipStream_t st) {
    const icv::Plan& p = pl->p;
    if (n < 1) return ICV_OK;
    const int W = p.W, n_cov = (int)p.cov_col.size(), R = (int)p.gv_run_j0.size();
    // the run table in LDS too where two workgroups per CU still fit (87 VGPRs allow no more than two anyway)
    const bool pk_lds = icv::gv_lds_bytes(W, R, pl->gv_mult_bytes, true) * 2 <= (size_t)icv::kLdsLimit;
    const size_t lds = icv::gv_lds_bytes(W, R, pl->gv_mult_bytes, pk_lds);
    if (lds <= (size_t)icv::kLdsLimit && pl->gv_fused_ok && !knobs().no_gene_fused) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(icv::k_gene_fused),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = (int)((size_t)icv::kLdsLimit / lds);
        if (per_cu > 2048 / icv::kGvThreads) per_cu = 2048 / icv::kGvThreads;  // 32 wavefronts per CU
        hipLaunchKernelGGL(icv::k_gene_fused, dim3((unsigned)cu_grid(pl, per_cu, n)), dim3(icv::kGvThreads), lds, st, win, ldw, n, W,
                           pl->d_gv_pk, pl->d_gv_mult, R, n_cov, pl->d_gv_col16, p.n_cols_all, thr,
                           chunksize > 0 ? chunksize : 1, row_phase, gene_out, ldg, pl->gv_mult_bytes, (int)pk_lds);
        HIP_TRY(hipGetLastError());
        return ICV_OK;
    }
    AsyncBuf b_gv, b_med;
    HIP_TRY(b_gv.alloc((size_t)n * (n_cov > 0 ? n_cov : 1) * sizeof(double), st));
    HIP_TRY(b_med.alloc((size_t)n * sizeof(double), st));
    double *gv = b_gv.as<double>(), *med = b_med.as<double>();
    {
        const int64_t total = n * (int64_t)p.n_cols_all;
        if (total > 0)
            hipLaunchKernelGGL(icv::k_fill_nan, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gene_out, n,
                               (int64_t)p.n_cols_all, ldg);
    }
    if (n_cov > 0) {
        for (int64_t r0 = 0; r0 < n; r0 += 32768) {
            const int64_t nr = (n - r0) < 32768 ? (n - r0) : 32768;
            dim3 grid((n_cov + 255) / 256, (unsigned)nr);
            hipLaunchKernelGGL(icv::k_gene_means, grid, dim3(256), 0, st, win + r0 * ldw, nr, (int)ldw, pl->d_cov_j0,
                               pl->d_cov_cnt, n_cov, gv + r0 * n_cov);
        }
        hipLaunchKernelGGL(icv::k_row_median, dim3((unsigned)n), dim3(256), 0, st, gv, n, n_cov, med);
        for (int64_t r0 = 0; r0 < n; r0 += 32768) {
            const int64_t nr = (n - r0) < 32768 ? (n - r0) : 32768;
            dim3 grid((n_cov + 255) / 256, (unsigned)nr);
            // chunk of row r0 + i: (r0 + i + row_phase) / chunksize relative to thr[0]
            hipLaunchKernelGGL(icv::k_gene_finish, grid, dim3(256), 0, st, gv + r0 * n_cov, med + r0, thr,
                               chunksize > 0 ? chunksize : 1, row_phase + r0, pl->d_cov_col, n_cov, gene_out + r0 * ldg,
                               ldg);
        }
    }
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}
}  // namespace

extern "C" {

int icv_infercnv_run(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi, double lfc_clip,
                     double dynamic_threshold, int64_t chunksize, int64_t row_phase, int32_t flags, float* out,
                     int64_t ldo, double* cell_median, double* cell_stats, double* thr, icv_profile* prof,
                     void* stream) {
    return icv_infercnv_run_finite(pl, m, ref_lo, ref_hi, lfc_clip, dynamic_threshold, chunksize, row_phase, flags, out,
                                   ldo, cell_median, cell_stats, thr, prof, nullptr, 0, nullptr, stream);
}

int icv_infercnv_run_windows(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi,
                             double lfc_clip, double dynamic_threshold, int64_t chunksize, int64_t row_phase,
                             int32_t flags, float* out, int64_t ldo, double* cell_median, double* cell_stats,
                             double* thr, icv_profile* prof, double* win_out, int64_t ldw, void* stream) {
    return icv_infercnv_run_finite(pl, m, ref_lo, ref_hi, lfc_clip, dynamic_threshold, chunksize, row_phase, flags, out,
                                   ldo, cell_median, cell_stats, thr, prof, win_out, ldw, nullptr, stream);
}

int icv_infercnv_run_finite(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi,
                            double lfc_clip, double dynamic_threshold, int64_t chunksize, int64_t row_phase,
                            int32_t flags, float* out, int64_t ldo, double* cell_median, double* cell_stats,
                            double* thr, icv_profile* prof, double* win_out, int64_t ldw,
                            const uint32_t* finite_words, void* stream) {
    if (finite_words && (reinterpret_cast<uintptr_t>(finite_words) & 15))
        return fail(ICV_ERR_INVALID, "finite_words must be 16-byte aligned");
    int rc = check_matrix(pl, m);
    if (rc) return rc;
    PLAN_BUSY_GUARD(pl);
    const bool do_thr = !std::isnan(dynamic_threshold);
    if (m->n_rows == 0) return ICV_OK;  // an empty shard: no cell, no chunk, nothing written
    if (!cell_median) return fail(ICV_ERR_INVALID, "cell_median is required");
    if (do_thr && (!thr || !chunk_args_ok(thr, chunksize, row_phase)))
        return fail(ICV_ERR_INVALID, "thr buffer / chunksize / row_phase invalid");
    if (win_out && ldw < pl->p.W) return fail(ICV_ERR_INVALID, "ldw < n_windows");
    if ((rc = ensure_device(pl))) return rc;
    PLAN_ENTER(stream);
    return run_steps(pl, m, ref_lo, ref_hi, lfc_clip, dynamic_threshold, chunksize, row_phase, flags, out, ldo,
                     cell_median, cell_stats, thr, prof, win_out, ldw, finite_words, stream);
}

int icv_gene_values_from_windows(icv_plan_t pl, const double* win, int64_t ldw, int64_t n_rows, const double* thr,
                                 int64_t chunksize, int64_t row_phase, double* gene_out, int64_t ldg, void* stream) {
    if (!pl) return fail(ICV_ERR_INVALID, "null plan");
    PLAN_BUSY_GUARD(pl);
    if (n_rows < 0 || (n_rows > 0 && (!win || !gene_out)) || ldw < pl->p.W || ldg < pl->p.n_cols_all)
        return fail(ICV_ERR_INVALID, "bad gene_values_from_windows arguments (null buffer, ldw < n_windows or ldg < n_cols)");
    if (!chunk_args_ok(thr, chunksize, row_phase)) return fail(ICV_ERR_INVALID, "chunksize / row_phase invalid");
    int rc;
    if ((rc = ensure_device(pl))) return rc;
    PLAN_ENTER(stream);
    return gene_from_windows(pl, win, ldw, n_rows, thr, chunksize, row_phase, gene_out, ldg,
                             static_cast<hipStream_t>(stream));
}

int icv_profile_begin(icv_plan_t pl) {
    if (!pl) return fail(ICV_ERR_INVALID, "null plan");
    for (auto& e : pl->prof_events) (void)hipEventDestroy(e);
    pl->prof_events.clear();
    pl->prof_deferred = true;
    return ICV_OK;
}

int icv_profile_collect(icv_plan_t pl, icv_profile* out, int32_t max_records, int32_t* n_records) {
    if (!pl || !n_records || (max_records > 0 && !out)) return fail(ICV_ERR_INVALID, "bad profile_collect arguments");
    const int n = (int)(pl->prof_events.size() / 4);
    int k = 0;
    for (int i = 0; i < n; ++i) {
        if (k < max_records) {
            if (int rc = read_profile(pl->prof_events.data() + 4 * i, &out[k])) return rc;
            ++k;
        }
    }
    for (auto& e : pl->prof_events) (void)hipEventDestroy(e);
    pl->prof_events.clear();
    pl->prof_deferred = false;
    *n_records = k;
    return ICV_OK;
}

int icv_gene_values(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi, double lfc_clip,
                    int32_t flags, const double* thr, int64_t chunksize, int64_t row_phase, double* gene_out,
                    int64_t ldg, void* stream) {
    int rc = check_matrix(pl, m);
    if (rc) return rc;
    PLAN_BUSY_GUARD(pl);
    if (!gene_out || ldg < m->n_cols) return fail(ICV_ERR_INVALID, "gene_out is null or ldg < n_cols");
    if (!chunk_args_ok(thr, chunksize, row_phase)) return fail(ICV_ERR_INVALID, "chunksize / row_phase invalid");
    if ((rc = ensure_device(pl))) return rc;
    PLAN_ENTER(stream);
    const int64_t n = m->n_rows;
    if (n < 1) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int W = pl->p.W;
    // ONE smoothing pass through the kernel the plain call takes (k_smooth_x16 / k_smooth_se write the float64 windows
    // beside x_res; other geometries: the generic kernel), then the fused gene kernel.  (A caller that also wants
    // X_cnv uses icv_infercnv_run_windows + icv_gene_values_from_windows: no second smoothing at all.)
    AsyncBuf b_out32, b_win, b_cmed;
    HIP_TRY(b_out32.alloc((size_t)n * W * sizeof(float), st));
    HIP_TRY(b_win.alloc((size_t)n * W * sizeof(double), st));
    HIP_TRY(b_cmed.alloc((size_t)n * sizeof(double), st));
    if ((rc = run_steps(pl, m, ref_lo, ref_hi, lfc_clip, std::nan(""), 1, 0, flags, b_out32.as<float>(), W,
                        b_cmed.as<double>(), nullptr, nullptr, nullptr, b_win.as<double>(), W, nullptr, stream)))
        return rc;
    return gene_from_windows(pl, b_win.as<double>(), W, n, thr, chunksize, row_phase, gene_out, ldg, st);
}

int icv_threshold_mask(icv_plan_t pl, const icv_matrix* m, const void* ref_lo, const void* ref_hi, double lfc_clip,
                       int32_t flags, const float* out, int64_t ldo, const double* cell_median, const double* thr,
                       int64_t chunksize, int64_t row_phase, uint64_t* mask, int64_t* row_nnz, void* stream) {
    int rc = check_matrix(pl, m);
    if (rc) return rc;
    PLAN_BUSY_GUARD(pl);
    if (!cell_median || !mask || !row_nnz || !chunk_args_ok(thr, chunksize, row_phase))
        return fail(ICV_ERR_INVALID, "bad threshold_mask arguments");
    if ((rc = ensure_device(pl))) return rc;
    PLAN_ENTER(stream);
    icv::KParams K;
    const icv::Layout* lay;
    if ((rc = fill_params(pl, m, ref_lo, ref_hi, lfc_clip, flags, const_cast<float*>(out), ldo,
                          const_cast<double*>(cell_median), nullptr, K, lay)))
        return rc;
    if (K.n_rows < 1) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_words = (pl->p.W + 63) / 64;
    const int64_t cs = thr ? chunksize : 1;
    auto* mk = reinterpret_cast<unsigned long long*>(mask);
    // streamed form (k_thr_mask_ring: rows through an LDS ring by LDS-DMA, one persistent workgroup per CU) where the
    // rows are 16-byte aligned and at least 1 KB; else one workgroup per row
    const icv::PackRing pr(pl->p.W);
    const bool ring = !knobs().no_mask_ring && pr.ok && (ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(mask) & 7) == 0;
    if (ring) {
        const int lds = pr.lds_bytes();
        const int64_t rounds = (K.n_rows + icv::kPmRows - 1) / icv::kPmRows;
        const unsigned gx = (unsigned)(rounds < pl->n_cu ? rounds : pl->n_cu);
        AsyncBuf ties;  // (row, wavefront part) pairs whose windows float32 could not decide
        if (thr) HIP_TRY(ties.alloc((size_t)K.n_rows * icv::kPmPerRow * sizeof(unsigned long long), st));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(icv::k_thr_mask_ring),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, icv::kPmLds));  // (per device: every call)
        hipLaunchKernelGGL(icv::k_thr_mask_ring, dim3(gx), dim3(icv::kPmThreads), lds, st, K, thr, cs, row_phase, mk, n_words,
                           row_nnz, pl->d_tie_n, ties.as<unsigned long long>());
        if (thr)
            by_matrix(m, [&](auto t, auto csr) {
                hipLaunchKernelGGL((icv::k_thr_mask_ties<decltype(t), decltype(csr)::value>), dim3(128), dim3(256), 0, st, K, thr,
                                   cs, row_phase, mk, n_words, row_nnz, pl->d_tie_n, ties.as<unsigned long long>());
            });
        HIP_TRY(hipGetLastError());
        return ICV_OK;
    }
    by_matrix(m, [&](auto t, auto csr) {
        hipLaunchKernelGGL((icv::k_thr_mask<decltype(t), decltype(csr)::value>), dim3((unsigned)K.n_rows), dim3(256), 0, st, K,
                           thr, cs, row_phase, mk, n_words, row_nnz);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_pack_geometry(int32_t n_windows, icv_pack_info* info) {
    if (!info || n_windows < 1) return fail(ICV_ERR_INVALID, "bad pack_geometry arguments");
    const icv::PackRing pr(n_windows);
    const icv::FillRing fr(n_windows);
    info->rows_per_round = icv::kPmRows;
    info->mask_streamed = pr.ok ? 1 : 0;
    info->mask_ring_slots = pr.ok ? pr.n_slots : 0;
    info->mask_lds_bytes = pr.ok ? pr.lds_bytes() : 0;
    info->mask_loads_in_flight = pr.ok ? (pr.n_slots - 1) * pr.per_loader : 0;
    info->fill_streamed = fr.ok ? 1 : 0;
    info->fill_ring_slots = fr.ok ? fr.n_slots : 0;
    info->fill_lds_bytes = fr.ok ? fr.lds_bytes() : 0;
    info->fill_loads_in_flight = fr.ok ? (fr.n_slots - 1) * (fr.per_loader + fr.n_extra) : 0;
    info->fill_stage_entries = fr.ok ? fr.cap : 0;
    return ICV_OK;
}

int icv_row_offsets(const int64_t* row_nnz, int64_t n_rows, int64_t* indptr, void* stream) {
    if ((!row_nnz && n_rows > 0) || !indptr || n_rows < 0) return fail(ICV_ERR_INVALID, "bad row_offsets arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned nb = (unsigned)((n_rows + icv::kScanBlock - 1) / icv::kScanBlock);
    AsyncBuf sums;
    HIP_TRY(sums.alloc((size_t)(nb ? nb : 1) * sizeof(int64_t), st));
    if (nb > 1) hipLaunchKernelGGL(icv::k_row_block_sums, dim3(nb), dim3(1024), 0, st, row_nnz, n_rows, sums.as<int64_t>());
    hipLaunchKernelGGL(icv::k_row_offsets, dim3(nb ? nb : 1), dim3(1024), 0, st, row_nnz, n_rows, sums.as<int64_t>(), indptr);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_csr_fill_masked(const float* x, int64_t n_rows, int32_t n_cols, int64_t ld, const uint64_t* mask,
                        const int64_t* indptr, int32_t* indices, double* data, void* stream) {
    if (!x || !mask || !indptr || !indices || !data || n_cols < 0 || ld < n_cols)
        return fail(ICV_ERR_INVALID, "bad csr_fill_masked arguments");
    if (n_rows < 1) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // streamed form (k_csr_fill_ring: rows, mask rows and row offsets through an LDS ring, one persistent workgroup per
    // CU) where the rows are 16-byte aligned and at least 1 KB; else one wavefront per row
    const icv::FillRing fr(n_cols);
    if (!knobs().no_fill_ring && fr.ok && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
        (reinterpret_cast<uintptr_t>(mask) & 7) == 0) {
        const int n_cu = current_cu_count();
        const int64_t rounds = (n_rows + icv::kPmRows - 1) / icv::kPmRows;
        const unsigned gx = (unsigned)(rounds < n_cu ? rounds : n_cu);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(icv::k_csr_fill_ring),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, icv::kPmLds));  // (per device: every call)
        hipLaunchKernelGGL(icv::k_csr_fill_ring, dim3(gx), dim3(icv::kPmThreads), fr.lds_bytes(), st, x, n_rows, n_cols, ld,
                           reinterpret_cast<const unsigned long long*>(mask), indptr, indices, data);
        HIP_TRY(hipGetLastError());
        return ICV_OK;
    }
    hipLaunchKernelGGL(icv::k_csr_fill_masked, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, x, n_rows, n_cols, ld,
                       reinterpret_cast<const unsigned long long*>(mask), (n_cols + 63) / 64, indptr, indices, data);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // extern "C"

// ---- Gram / distance tile jobs (icv_corr.hpp) -------------------------------------------------------
namespace {
struct GramWork {  // device side of one k_gram_mfma launch: the super-tile descriptors
    char* buf = nullptr;
    ~GramWork() { (void)hipFree(buf); }
};

template <bool DIST, bool SYM>
int launch_gram(hipStream_t st, GramWork& w, const float* z, int kz, const double* norm,
                const std::vector<icv::GramSuper>& supers, int64_t row_end, int64_t col_end, float* c_dir,
                int64_t ld_dir, float* c_mir, int64_t ld_mir) {
    if (supers.empty()) return ICV_OK;
    HIP_TRY(hipMalloc((void**)&w.buf, supers.size() * sizeof(icv::GramSuper)));
    HIP_TRY(hipMemcpyAsync(w.buf, supers.data(), supers.size() * sizeof(icv::GramSuper), hipMemcpyHostToDevice, st));
    icv::GramJob J;
    J.supers = reinterpret_cast<const icv::GramSuper*>(w.buf);
    J.n_supers = (int)supers.size();
    J.row_end = row_end;
    J.col_end = col_end;
    J.c_dir = c_dir;
    J.ld_dir = ld_dir;
    J.c_mir = c_mir;
    J.ld_mir = ld_mir;
    const unsigned grid = 512u * (unsigned)((supers.size() + 7) / 8);
    hipLaunchKernelGGL((icv::k_gram_mfma<DIST, SYM>), dim3(grid), dim3(256), 0, st, z, kz, norm, J);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// super-tiles of the full symmetric n x n result (upper triangle, row-major)
std::vector<icv::GramSuper> gram_supers_sym(int64_t n, int64_t ld) {
    const int64_t ss = (int64_t)icv::GT * icv::GSUPER;
    const int64_t ns = (n + ss - 1) / ss;
    std::vector<icv::GramSuper> v;
    v.reserve((size_t)(ns * (ns + 1) / 2));
    for (int64_t sy = 0; sy < ns; ++sy)
        for (int64_t sx = sy; sx < ns; ++sx)
            v.push_back({(int)(sy * ss), (int)(sx * ss), sy * ss * ld + sx * ss, sx * ss * ld + sy * ss});
    return v;
}
}  // namespace

extern "C" {

int icv_corr_iqr(const float* x, int64_t n, int32_t k, int64_t ld, double* h_iqr, void* stream) {
    if (!x || !h_iqr || n < 2 || k < 1 || ld < k) return fail(ICV_ERR_INVALID, "bad corr_iqr arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int kz = icv::round_up(k, icv::GK);
    // stream-ordered temporaries from the device's pool (kept between calls up to AsyncBuf's threshold: a fresh
    // hipMalloc of the n x n matrix costs tens of milliseconds on a box whose VRAM has not been touched yet)
    AsyncBuf z_b, c_b, cnt_b;
    HIP_TRY(z_b.alloc((size_t)n * kz * sizeof(float), st));
    HIP_TRY(c_b.alloc((size_t)n * n * sizeof(float), st));
    HIP_TRY(cnt_b.alloc((4 * 2048 + 1) * sizeof(unsigned long long), st));
    float *z = z_b.as<float>(), *c = c_b.as<float>();
    unsigned long long* d_cnt = cnt_b.as<unsigned long long>();
    hipLaunchKernelGGL(icv::k_row_normalize, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, n, k, ld, z, kz);
    GramWork gw;
    if (int rc = launch_gram<false, true>(st, gw, z, kz, nullptr, gram_supers_sym(n, n), n, n, c, n, c, n)) return rc;
    // the 25 % and 75 % percentiles interpolate between order statistics floor(pos), floor(pos) + 1
    const double m1 = (double)n * (double)n - 1.0;
    const double pos[2] = {0.25 * m1, 0.75 * m1};
    unsigned long long target[4];
    for (int q = 0; q < 2; ++q) {
        target[2 * q] = (unsigned long long)std::floor(pos[q]);
        target[2 * q + 1] = target[2 * q] + 1 < (unsigned long long)(m1 + 1.0) ? target[2 * q] + 1 : target[2 * q];
    }
    // the keys of ranks target[0..3] by radix selection on the ordered 32-bit keys (exact): 11 + 11 + 10 bits, one pass
    // over the matrix each (k_key_hist; targets that share their higher bits share a histogram).  Round 5 bisected with
    // k_count_le4: 33 passes, half of ithcna's time at 25 000 cells per group.
    unsigned lo[4] = {0, 0, 0, 0};
    const int64_t m = n * n;
    int64_t grid = (m + 255) / 256;
    if (grid > 4096) grid = 4096;
    bool any_nan = false;
    {
        std::vector<unsigned long long> h(4 * 2048 + 1);
        unsigned long long below[4] = {0, 0, 0, 0};  // elements whose key is below the target's current prefix range
        unsigned prefix[4] = {0, 0, 0, 0};
        const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
        for (int pass = 0; pass < 3 && !any_nan; ++pass) {
            const unsigned himask = pass == 0 ? 0u : ~((1u << (shifts[pass] + bits[pass])) - 1u);
            // distinct prefixes -> histograms
            unsigned pq[4] = {0, 0, 0, 0};
            int which[4], nq = 0;
            for (int q = 0; q < 4; ++q) {
                int f = -1;
                for (int k = 0; k < nq; ++k)
                    if (pq[k] == (prefix[q] & himask)) f = k;
                if (f < 0) {
                    pq[nq] = prefix[q] & himask;
                    f = nq++;
                }
                which[q] = f;
            }
            HIP_TRY(hipMemsetAsync(d_cnt, 0, (4 * 2048 + 1) * sizeof(unsigned long long), st));
            hipLaunchKernelGGL(icv::k_key_hist, dim3((unsigned)grid), dim3(256), 0, st, c, m, shifts[pass], bits[pass], himask,
                               pq[0], pq[1], pq[2], pq[3], nq, d_cnt);
            HIP_TRY(hipMemcpyAsync(h.data(), d_cnt, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h[4 * 2048]) {
                any_nan = true;
                break;
            }
            for (int q = 0; q < 4; ++q) {
                const unsigned long long* hq = h.data() + (size_t)which[q] * 2048;
                unsigned long long run = below[q];
                unsigned d = 0;
                const unsigned nd = 1u << bits[pass];
                for (; d + 1 < nd; ++d) {
                    if (run + hq[d] > target[q]) break;
                    run += hq[d];
                }
                below[q] = run;
                prefix[q] |= d << shifts[pass];
            }
        }
        for (int q = 0; q < 4; ++q) lo[q] = prefix[q];
    }
    if (any_nan) {
        *h_iqr = std::nan("");
        return ICV_OK;
    }
    double qv[2];
    for (int q = 0; q < 2; ++q) {
        const double a = (double)icv::from_ordered_key32(lo[2 * q]), b = (double)icv::from_ordered_key32(lo[2 * q + 1]);
        const double t = pos[q] - std::floor(pos[q]);
        const double d = b - a;
        qv[q] = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;  // numpy's _lerp
    }
    *h_iqr = qv[1] - qv[0];
    return ICV_OK;
}

}  // extern "C"

namespace {
// centred float32 copy of the points (distances are translation invariant) + float64 squared norms
struct CentredPoints {
    float* z = nullptr;
    double* work = nullptr;  // partial[n_slabs * d] | mean[d] | norm[n]
    double* norm = nullptr;
    int kz = 0;
    ~CentredPoints() {
        (void)hipFree(z);
        (void)hipFree(work);
    }
};
int centre_points(hipStream_t st, const float* x, int64_t n, int32_t d, int64_t ld, CentredPoints& c) {
    c.kz = icv::round_up(d, icv::GK);
    const int n_slabs = (int)std::min<int64_t>(256, (n + 63) / 64);
    HIP_TRY(hipMalloc((void**)&c.z, (size_t)n * c.kz * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c.work, ((size_t)n_slabs * d + d + n) * sizeof(double)));
    double *partial = c.work, *mean = c.work + (size_t)n_slabs * d;
    c.norm = mean + d;
    const unsigned gd = (unsigned)((d + 255) / 256);
    hipLaunchKernelGGL(icv::k_colsum_slabs, dim3(gd, n_slabs), dim3(256), 0, st, x, n, d, ld, n_slabs, partial);
    hipLaunchKernelGGL(icv::k_colmean_finish, dim3(gd), dim3(256), 0, st, partial, n, d, n_slabs, mean);
    hipLaunchKernelGGL(icv::k_center_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, n, d, ld, mean, c.z, c.kz,
                       c.norm);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}
}  // namespace

extern "C" {

int icv_pairwise_sqeuclidean(const float* x, int64_t n, int32_t d, int64_t ld, int64_t row_begin, int64_t row_end,
                             float* out, int64_t ldo, void* stream) {
    if (!x || !out || n < 1 || d < 1 || ld < d || ldo < n || row_begin < 0 || row_end > n || row_begin > row_end)
        return fail(ICV_ERR_INVALID, "bad pairwise arguments");
    if (row_begin == row_end) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CentredPoints c;
    if (int rc = centre_points(st, x, n, d, ld, c)) return rc;
    GramWork gw;
    if (row_begin == 0 && row_end == n) {
        if (int rc = launch_gram<true, true>(st, gw, c.z, c.kz, c.norm, gram_supers_sym(n, ldo), n, n, out, ldo, out, ldo))
            return rc;
    } else {  // a row block against all columns
        const int64_t ss = (int64_t)icv::GT * icv::GSUPER;
        std::vector<icv::GramSuper> v;
        for (int64_t r0 = row_begin; r0 < row_end; r0 += ss)
            for (int64_t c0 = 0; c0 < n; c0 += ss) v.push_back({(int)r0, (int)c0, (r0 - row_begin) * ldo + c0, 0});
        if (int rc = launch_gram<true, false>(st, gw, c.z, c.kz, c.norm, v, row_end, n, out, ldo, out, ldo)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));  // the temporaries are freed on return
    return ICV_OK;
}

int icv_pairwise_sqeuclidean_tiles(const float* x, int64_t n, int32_t d, int64_t ld, int32_t n_tiles,
                                   const int32_t* h_row0, const int32_t* h_col0, const int64_t* h_dir_off,
                                   const int64_t* h_mir_off, float* dir, int64_t ld_dir, float* mir, int64_t ld_mir,
                                   void* stream) {
    static_assert(ICV_SUPER_ROWS == icv::GT * icv::GSUPER, "super-tile size");
    if (!x || n < 1 || d < 1 || ld < d || n_tiles < 0) return fail(ICV_ERR_INVALID, "bad pairwise tile arguments");
    if (n_tiles == 0) return ICV_OK;
    if (!h_row0 || !h_col0 || !h_dir_off || !h_mir_off || !dir || !mir)
        return fail(ICV_ERR_INVALID, "bad pairwise tile arguments");
    std::vector<icv::GramSuper> v((size_t)n_tiles);
    for (int32_t k = 0; k < n_tiles; ++k) {
        if (h_row0[k] < 0 || h_row0[k] % ICV_SUPER_ROWS || h_col0[k] % ICV_SUPER_ROWS || h_col0[k] < h_row0[k] ||
            h_col0[k] >= n)
            return fail(ICV_ERR_INVALID, "pairwise tiles: origins must be multiples of ICV_SUPER_ROWS on or above the diagonal");
        v[(size_t)k] = {h_row0[k], h_col0[k], h_dir_off[k], h_mir_off[k]};
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    CentredPoints c;
    if (int rc = centre_points(st, x, n, d, ld, c)) return rc;
    GramWork gw;
    if (int rc = launch_gram<true, true>(st, gw, c.z, c.kz, c.norm, v, n, n, dir, ld_dir, mir, ld_mir)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return ICV_OK;
}

}  // extern "C"

// ---- Ward rounds: device bookkeeping shared by the one-call and the step-wise entry points ---------------
// Two column layouts (icv_ward.hpp / icv_ward_strip.hpp): "strip" when the row stride leaves n / 2 spare columns
// (merged clusters get new, consecutive columns: dense strip updates), "in place" otherwise.
struct icv_ward_s {
    int64_t n = 0, ld = 0;
    int cap = 0;         // usable columns of a row (strip layout)
    bool strip = false;
    char* buf = nullptr;
    int *live, *cstate, *size_old, *size_new, *nn, *log_i, *log_j, *log_size, *act, *pslot, *vrow, *ulist;
    float *pair_d, *dmin, *log_d;
    unsigned char *alive, *qmask;
    int4 *mdesc, *mpos;
    icv::WardStripCounts* counts;
    icv::WardPos pos{};
    int *sr_local = nullptr, *sr_global = nullptr;  // device copies (sharded matrices)
    icv::WardMap map{nullptr, nullptr, 10, 0};
    icv::WardStripCounts h{0, 0, 0, 0, 0, 0, 0, 0};  // after the last icv_ward_pairs
    int rounds = 0;
    ~icv_ward_s() { (void)hipFree(buf); }
    bool vec_ok(const void* D, int64_t ld_) const { return (ld_ % 4 == 0) && ((reinterpret_cast<uintptr_t>(D) & 15) == 0); }
    // stream over all columns, or gather over the live list?
    bool dense(const void* D, int64_t ld_, int width) const { return vec_ok(D, ld_) && (int64_t)h.n_live * 4 >= width; }
    int merged_begin() const { return h.n_merges - h.n_pairs; }
};

namespace {
int ward_create(int64_t n, const int32_t* sr_local, int32_t n_super, int32_t super_shift, int64_t ld, bool spare,
                hipStream_t st, icv_ward_s** out) {
    if (n < 2 || n > 0x7fffffff / 2 || !out || ld < n) return fail(ICV_ERR_INVALID, "bad ward arguments");
    if (spare && (ld % 4 != 0 || ld < n + (n + 1) / 2))
        return fail(ICV_ERR_INVALID, "ward: spare columns need a row stride that is a multiple of 4 and >= n + (n + 1) / 2");
    if (sr_local && (n_super < 1 || super_shift < 2 || super_shift > 20 || ((int64_t)n_super << super_shift) < n))
        return fail(ICV_ERR_INVALID, "bad ward storage map");
    std::unique_ptr<icv_ward_s> w(new icv_ward_s);
    w->n = n;
    w->ld = ld;
    // the caller says whether columns [n, ld) of every row are the rounds' to use (never inferred from the stride: a
    // column slice of a wider buffer has a large stride too); ICV_WARD_IN_PLACE: developer knob, the other layout
    w->strip = spare && !knobs().ward_in_place;
    w->cap = w->strip ? (int)std::min<int64_t>(ld, 2 * n) : (int)n;
    const size_t arr = ((size_t)n * 4 + 255) / 256 * 256;
    const size_t parr = ((size_t)w->cap * 4 + 255) / 256 * 256;  // arrays indexed by column position
    const size_t map_bytes = sr_local ? ((size_t)n_super * 8 + 255) / 256 * 256 : 0;
    // 16 slot-indexed arrays + 2 x 4 (merge descriptors) + slot_pos; 6 position-indexed arrays; counters; storage map
    HIP_TRY(hipMalloc((void**)&w->buf, arr * 25 + parr * 6 + 512 + map_bytes));
    char* b = w->buf;
    auto take = [&](size_t bytes) {
        char* p = b;
        b += bytes;
        return p;
    };
    w->live = (int*)take(arr);
    w->cstate = (int*)take(arr);
    w->pair_d = (float*)take(arr);
    w->size_old = (int*)take(arr);
    w->size_new = (int*)take(arr);
    w->nn = (int*)take(arr);
    w->dmin = (float*)take(arr);
    w->log_i = (int*)take(arr);
    w->log_j = (int*)take(arr);
    w->log_d = (float*)take(arr);
    w->log_size = (int*)take(arr);
    w->alive = (unsigned char*)take(arr);
    w->act = (int*)take(arr);
    w->pslot = (int*)take(arr);
    w->vrow = (int*)take(arr);
    w->ulist = (int*)take(arr);
    w->mdesc = (int4*)take(arr * 4);  // n x 16 bytes: one packed descriptor per merge
    w->mpos = (int4*)take(arr * 4);
    w->pos.slot_pos = (int*)take(arr);
    w->qmask = (unsigned char*)take(parr);
    w->pos.pos_slot = (int*)take(parr);
    w->pos.palive = (unsigned char*)take(parr);
    w->pos.pstate = (int*)take(parr);
    w->pos.psize = (int*)take(parr);
    w->pos.newpos = (int*)take(parr);
    w->counts = (icv::WardStripCounts*)take(256);
    if (sr_local) {
        // local super-row index per global super-row and its inverse
        std::vector<int> inv;
        for (int g = 0; g < n_super; ++g)
            if (sr_local[g] >= 0) {
                if ((size_t)sr_local[g] >= inv.size()) inv.resize((size_t)sr_local[g] + 1, -1);
                inv[(size_t)sr_local[g]] = g;
            }
        for (int v : inv)
            if (v < 0) return fail(ICV_ERR_INVALID, "ward storage map: local super-rows must be 0 .. k-1");
        w->sr_local = (int*)b;
        w->sr_global = w->sr_local + n_super;
        HIP_TRY(hipMemcpyAsync(w->sr_local, sr_local, (size_t)n_super * 4, hipMemcpyHostToDevice, st));
        if (!inv.empty())
            HIP_TRY(hipMemcpyAsync(w->sr_global, inv.data(), inv.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        int64_t n_local = 0;
        for (size_t l = 0; l < inv.size(); ++l) {
            const int64_t r0 = (int64_t)inv[l] << super_shift;
            n_local = std::max<int64_t>(n_local, ((int64_t)l << super_shift) + std::min<int64_t>(n - r0, (int64_t)1 << super_shift));
        }
        w->map = icv::WardMap{w->sr_local, w->sr_global, super_shift, (int)n_local};
    } else {
        w->map = icv::WardMap{nullptr, nullptr, 10, (int)n};
    }
    // both layouts start from the same state: width n, every row to be searched
    hipLaunchKernelGGL(icv::k_ward_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, w->live,
                       w->cstate, w->qmask, w->size_old, w->size_new, w->alive, w->act,
                       reinterpret_cast<icv::WardCounts*>(w->counts));
    if (w->strip)
        hipLaunchKernelGGL(icv::k_ward_init_s, dim3((unsigned)((w->cap + 255) / 256)), dim3(256), 0, st, (int)n, w->cap,
                           w->pos, w->ulist, w->qmask, w->counts);
    HIP_TRY(hipGetLastError());
    w->h = icv::WardStripCounts{(int)n, 0, 0, (int)n, (int)n, (int)n, 0, (int)n};
    *out = w.release();
    return ICV_OK;
}

int ward_check_ld(const icv_ward_s* w, int64_t ld, const void* D = nullptr) {
    if (ld != w->ld) return fail(ICV_ERR_INVALID, "ward: the row stride differs from the one given to icv_ward_create");
    if (w->strip && D && (reinterpret_cast<uintptr_t>(D) & 15))
        return fail(ICV_ERR_INVALID, "ward: a matrix with spare columns must be 16-byte aligned");
    return ICV_OK;
}

int ward_merge(icv_ward_s* w, float* D, int64_t ld, const float* stage, int64_t ld_stage, const int32_t* h_pslot,
               bool scatter, hipStream_t st) {
    if (int rc = ward_check_ld(w, ld, D)) return rc;
    if (w->h.n_pairs < 1) return ICV_OK;
    const int mb = w->merged_begin();
    if (h_pslot) HIP_TRY(hipMemcpyAsync(w->pslot, h_pslot, (size_t)w->h.n_pairs * 4, hipMemcpyHostToDevice, st));
    const icv::WardPairView V{w->mdesc + mb, w->log_d + mb, h_pslot ? w->pslot : nullptr, stage, ld_stage};
    const bool stage_ok = !h_pslot || ((ld_stage % 4 == 0) && ((reinterpret_cast<uintptr_t>(stage) & 15) == 0));
    const dim3 grid((unsigned)w->h.n_pairs), block(256);
    if (w->strip) {
        if (w->dense(D, ld, w->h.width_prev) && stage_ok)
            hipLaunchKernelGGL(icv::k_ward_merge_s<true>, grid, block, 0, st, D, ld, w->h.width_prev, w->live, w->h.n_live,
                               w->cstate, V, w->mpos + mb, w->h.n_pairs, w->pos, w->map, w->nn, w->dmin);
        else
            hipLaunchKernelGGL(icv::k_ward_merge_s<false>, grid, block, 0, st, D, ld, w->h.width_prev, w->live, w->h.n_live,
                               w->cstate, V, w->mpos + mb, w->h.n_pairs, w->pos, w->map, w->nn, w->dmin);
        if (scatter && w->h.n_unmerged > 0) {  // one GPU: the strip update straight from the new rows
            const dim3 g2((unsigned)((w->h.n_pairs + 63) / 64), (unsigned)((w->h.n_unmerged + 63) / 64));
            hipLaunchKernelGGL(icv::k_ward_push, g2, block, 0, st, D, ld, w->h.width_prev, w->mdesc + mb, w->h.n_pairs,
                               w->ulist, w->h.n_unmerged, w->pos.slot_pos);
        }
    } else if (w->dense(D, ld, (int)w->n) && stage_ok) {
        hipLaunchKernelGGL(icv::k_ward_merge<true>, grid, block, 0, st, D, ld, (int)w->n, w->live, w->h.n_live, w->cstate,
                           V, w->pair_d, w->size_old, w->size_new, w->map, scatter, w->nn, w->dmin);
    } else {
        hipLaunchKernelGGL(icv::k_ward_merge<false>, grid, block, 0, st, D, ld, (int)w->n, w->live, w->h.n_live, w->cstate,
                           V, w->pair_d, w->size_old, w->size_new, w->map, scatter, w->nn, w->dmin);
    }
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int ward_scan(icv_ward_s* w, const float* D, int64_t ld, hipStream_t st) {
    if (int rc = ward_check_ld(w, ld, D)) return rc;
    if (w->h.n_act < 1) return ICV_OK;
    const dim3 grid((unsigned)w->h.n_act), block(256);
    if (w->strip) {
        if (w->dense(D, ld, w->h.width))
            hipLaunchKernelGGL(icv::k_ward_scan_s<true>, grid, block, 0, st, D, ld, w->h.width, w->act, w->live,
                               w->h.n_live, w->qmask, w->pos, w->map, w->nn, w->dmin);
        else
            hipLaunchKernelGGL(icv::k_ward_scan_s<false>, grid, block, 0, st, D, ld, w->h.width, w->act, w->live,
                               w->h.n_live, w->qmask, w->pos, w->map, w->nn, w->dmin);
    } else if (w->dense(D, ld, (int)w->n)) {
        hipLaunchKernelGGL(icv::k_ward_scan<true>, grid, block, 0, st, D, ld, (int)w->n, w->act, w->live, w->h.n_live,
                           w->qmask, w->map, w->nn, w->dmin);
    } else {
        hipLaunchKernelGGL(icv::k_ward_scan<false>, grid, block, 0, st, D, ld, (int)w->n, w->act, w->live, w->h.n_live,
                           w->qmask, w->map, w->nn, w->dmin);
    }
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int ward_read_counts(icv_ward_s* w, hipStream_t st) {
    if (w->strip) {
        HIP_TRY(hipMemcpyAsync(&w->h, w->counts, sizeof(w->h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        icv::WardCounts c;
        HIP_TRY(hipMemcpyAsync(&c, w->counts, sizeof(c), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        w->h = icv::WardStripCounts{c.n_live, c.n_merges, c.n_pairs, c.n_act, (int)w->n, (int)w->n, 0, 0};
    }
    return ICV_OK;
}

// in-place compaction of the alive columns of the alive local rows (strip layout)
int ward_compact(icv_ward_s* w, float* D, int64_t ld, hipStream_t st) {
    if (int rc = ward_check_ld(w, ld, D)) return rc;
    if (!w->strip) return ICV_OK;
    hipLaunchKernelGGL(icv::k_ward_compact_map, dim3(1), dim3(1024), 0, st, w->cap, w->pos, w->qmask, w->counts);
    if (w->h.n_live > 0 && w->map.n_local > 0)
        hipLaunchKernelGGL(icv::k_ward_compact_rows, dim3((unsigned)w->h.n_live), dim3(256), 0, st, D, ld, w->h.width,
                           w->live, w->pos.newpos, w->map);
    HIP_TRY(hipGetLastError());
    w->h.width_prev = w->h.width;
    w->h.width = w->h.n_live;
    w->h.need_compact = 0;
    return ICV_OK;
}

// reciprocal pairs of the round; strip layout: compacts first when fewer than half of the positions are alive,
// and again (then it must fit) when the round's new columns would not fit the spare region.  all_active (the pass
// that lists every row after a round without a pair) is bookkeeping only and is not counted as a round, for the
// one-call and the step-wise entry points alike.
int ward_pairs(icv_ward_s* w, float* D, int64_t ld, bool all_active, hipStream_t st) {
    if (!w->strip) {
        hipLaunchKernelGGL(icv::k_ward_pairs, dim3(1), dim3(1024), 0, st, (int)w->n, w->live, w->cstate, w->qmask, w->mdesc,
                           w->pair_d, w->size_old, w->size_new, w->alive, w->nn, w->dmin, w->log_i, w->log_j, w->log_d,
                           w->log_size, w->act, all_active ? 1 : 0, reinterpret_cast<icv::WardCounts*>(w->counts));
        HIP_TRY(hipGetLastError());
        if (!all_active) ++w->rounds;
        return ward_read_counts(w, st);
    }
    {
        // developer knob: compaction threshold (positions per alive column), default 2
        const double kx = knobs().ward_compact_x;
        const double thr = kx >= 1.05 ? kx : 2.0;
        if ((double)w->h.width > thr * (double)w->h.n_live && w->h.width > 4096)
            if (int rc = ward_compact(w, D, ld, st)) return rc;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int span = std::max<int>((int)w->n, w->cap);
        hipLaunchKernelGGL(icv::k_ward_prep_s, dim3((unsigned)((span + 255) / 256)), dim3(256), 0, st, (int)w->n, w->cstate,
                           w->size_old, w->size_new, w->alive, w->pos, w->counts);
        hipLaunchKernelGGL(icv::k_ward_pairs_s, dim3(1), dim3(1024), 0, st, (int)w->n, w->cap, w->live, w->cstate,
                           w->mdesc, w->mpos, w->pair_d, w->size_old, w->size_new, w->alive, w->nn, w->dmin, w->log_i,
                           w->log_j, w->log_d, w->log_size, w->act, w->ulist, all_active ? 1 : 0, w->pos, w->counts);
        hipLaunchKernelGGL(icv::k_ward_qmask_s, dim3((unsigned)(((w->cap + 3) / 4 + 255) / 256)), dim3(256), 0, st, w->cap,
                           w->pos.palive, w->qmask);
        HIP_TRY(hipGetLastError());
        const int width_before = w->h.width;
        if (int rc = ward_read_counts(w, st)) return rc;
        if (!w->h.need_compact) {
            if (!all_active) ++w->rounds;
            return ICV_OK;
        }
        if (attempt == 1) break;
        // nothing was committed: the counters other than need_compact are those of the previous round
        w->h.width = width_before;
        if (int rc = ward_compact(w, D, ld, st)) return rc;
    }
    return fail(ICV_ERR_UNSUPPORTED, "ward_pairs: the spare columns do not hold one round");
}

// merge log -> scipy linkage matrix: monotone heights, stable sort, union-find relabelling
int ward_finish(icv_ward_s* w, double* h_linkage) {
    const int64_t n = w->n;
    const size_t m = (size_t)n - 1;
    if ((size_t)w->h.n_merges != m) return fail(ICV_ERR_INVALID, "ward_finish: the rounds are not complete");
    std::vector<int> li(m), lj(m), ls(m);
    std::vector<float> ldq(m);
    HIP_TRY(hipMemcpy(li.data(), w->log_i, m * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lj.data(), w->log_j, m * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ls.data(), w->log_size, m * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ldq.data(), w->log_d, m * 4, hipMemcpyDeviceToHost));
    std::vector<double> height(m), slot_h((size_t)n, 0.0);
    for (size_t p = 0; p < m; ++p) {
        double h = std::sqrt((double)ldq[p]);
        h = std::max(h, std::max(slot_h[li[p]], slot_h[lj[p]]));  // a parent never sorts before its children
        height[p] = h;
        slot_h[li[p]] = h;
    }
    std::vector<size_t> order(m);
    for (size_t p = 0; p < m; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return height[a] < height[b]; });
    std::vector<int64_t> cluster((size_t)n);  // current scipy id of the cluster kept in each slot
    for (int64_t s = 0; s < n; ++s) cluster[s] = s;
    for (size_t q = 0; q < m; ++q) {
        const size_t p = order[q];
        const int64_t a = cluster[li[p]], b = cluster[lj[p]];
        h_linkage[4 * q + 0] = (double)std::min(a, b);
        h_linkage[4 * q + 1] = (double)std::max(a, b);
        h_linkage[4 * q + 2] = height[p];
        h_linkage[4 * q + 3] = (double)ls[p];
        cluster[li[p]] = n + (int64_t)q;
    }
    return ICV_OK;
}
}  // namespace

extern "C" {

int icv_ward_linkage(float* dist_sq, int64_t n, int64_t ld, int32_t spare_columns, double* h_linkage,
                     int32_t* h_rounds, void* stream) {
    if (!dist_sq || !h_linkage || n < 1 || ld < n || n > 0x7fffffff / 2)
        return fail(ICV_ERR_INVALID, "bad ward_linkage arguments");
    if (h_rounds) *h_rounds = 0;
    if (n == 1) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    icv_ward_s* raw = nullptr;
    if (int rc = ward_create(n, nullptr, 0, 0, ld, spare_columns != 0, st, &raw)) return rc;
    std::unique_ptr<icv_ward_s> w(raw);
    bool retry = false;
    while (w->h.n_live > 1) {
        if (int rc = ward_merge(w.get(), dist_sq, ld, nullptr, 0, nullptr, true, st)) return rc;
        if (int rc = ward_scan(w.get(), dist_sq, ld, st)) return rc;
        if (int rc = ward_pairs(w.get(), dist_sq, ld, false, st)) return rc;
        if (w->h.n_pairs < 1) {
            // No reciprocal pair: possible only when cached neighbours of TIED distances point in a cycle (fresh
            // neighbours under one total order always contain a reciprocal pair).  List every live row, search
            // them all again, and give up if that does not help (non-finite distances).
            if (retry) return fail(ICV_ERR_INVALID, "ward_linkage: distances are not finite");
            retry = true;
            if (int rc = ward_pairs(w.get(), dist_sq, ld, true, st)) return rc;
            if (w->h.n_pairs > 0) retry = false;
        } else {
            retry = false;
        }
    }
    if (h_rounds) *h_rounds = w->rounds;
    return ward_finish(w.get(), h_linkage);
}

int icv_ward_create(int64_t n, const int32_t* sr_local, int32_t n_super, int32_t super_shift, int64_t ld,
                    int32_t spare_columns,
                    icv_ward_t* out, void* stream) {
    return ward_create(n, sr_local, n_super, super_shift, ld, spare_columns != 0, static_cast<hipStream_t>(stream), out);
}
void icv_ward_destroy(icv_ward_t w) { delete w; }

int icv_ward_merge(icv_ward_t w, float* d_local, int64_t ld, const float* stage, int64_t ld_stage,
                   const int32_t* h_pslot, int32_t scatter, void* stream) {
    if (!w || !d_local) return fail(ICV_ERR_INVALID, "bad ward_merge arguments");
    return ward_merge(w, d_local, ld, stage, ld_stage, h_pslot, scatter != 0, static_cast<hipStream_t>(stream));
}

int icv_ward_gather(icv_ward_t w, const float* d_local, int64_t ld, const int64_t* d_rows, int32_t n_rows,
                    const int32_t* d_slots, int32_t n_slots, float* out, int64_t ldo, void* stream) {
    if (!w) return fail(ICV_ERR_INVALID, "bad ward_gather arguments");
    if (int rc = ward_check_ld(w, ld)) return rc;
    if (n_rows < 1 || n_slots < 1) return ICV_OK;
    if (!d_local || !d_rows || !d_slots || !out || ldo < n_slots) return fail(ICV_ERR_INVALID, "bad ward_gather arguments");
    hipLaunchKernelGGL(icv::k_ward_gather, dim3((unsigned)((n_slots + 255) / 256), (unsigned)n_rows), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_local, ld, d_rows, d_slots, n_slots,
                       w->strip ? w->pos.slot_pos : nullptr, w->strip ? w->h.width : (int)w->n, out, ldo);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_ward_scatter(icv_ward_t w, float* d_local, int64_t ld, const float* v, int64_t ldv, const int32_t* h_vrow_p,
                     int32_t n_v, void* stream) {
    if (!w || !d_local || n_v < 0 || n_v > w->n) return fail(ICV_ERR_INVALID, "bad ward_scatter arguments");
    if (int rc = ward_check_ld(w, ld)) return rc;
    if (n_v == 0 || w->map.n_local < 1) return ICV_OK;
    if (!v || !h_vrow_p || ldv < w->map.n_local || n_v != w->h.n_pairs)
        return fail(ICV_ERR_INVALID, "bad ward_scatter arguments (one row per merge of the round)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int mb = w->merged_begin();
    if (w->strip) {
        std::vector<int> inv((size_t)n_v, -1);  // merge index -> row of v
        for (int q = 0; q < n_v; ++q) {
            if (h_vrow_p[q] < 0 || h_vrow_p[q] >= n_v || inv[(size_t)h_vrow_p[q]] >= 0)
                return fail(ICV_ERR_INVALID, "ward_scatter: h_vrow_p must be a permutation of the round's merges");
            inv[(size_t)h_vrow_p[q]] = q;
        }
        HIP_TRY(hipMemcpyAsync(w->vrow, inv.data(), (size_t)n_v * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // inv is a temporary
        const dim3 grid((unsigned)((n_v + 63) / 64), (unsigned)((w->map.n_local + 63) / 64));
        hipLaunchKernelGGL(icv::k_ward_scatter_s, grid, dim3(256), 0, st, d_local, ld, w->h.width_prev, v, ldv, w->vrow, n_v,
                           w->cstate, w->map);
    } else {
        std::vector<int> slots((size_t)n_v);
        std::vector<int> li((size_t)n_v);
        HIP_TRY(hipMemcpyAsync(li.data(), w->log_i + mb, (size_t)n_v * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int q = 0; q < n_v; ++q) {
            if (h_vrow_p[q] < 0 || h_vrow_p[q] >= n_v) return fail(ICV_ERR_INVALID, "ward_scatter: bad merge index");
            slots[(size_t)q] = li[(size_t)h_vrow_p[q]];
        }
        HIP_TRY(hipMemcpyAsync(w->vrow, slots.data(), (size_t)n_v * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        hipLaunchKernelGGL(icv::k_ward_scatter, dim3((unsigned)((w->map.n_local + 255) / 256), (unsigned)n_v), dim3(256), 0,
                           st, d_local, ld, v, ldv, w->vrow, w->cstate, w->map);
    }
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_ward_scan(icv_ward_t w, const float* d_local, int64_t ld, void* stream) {
    if (!w || !d_local) return fail(ICV_ERR_INVALID, "bad ward_scan arguments");
    return ward_scan(w, d_local, ld, static_cast<hipStream_t>(stream));
}

int icv_ward_pack_nn(icv_ward_t w, int32_t* d_nn, float* d_dmin, void* stream) {
    if (!w || !d_nn || !d_dmin) return fail(ICV_ERR_INVALID, "bad ward_pack_nn arguments");
    const int k = w->h.n_pairs + w->h.n_act;
    if (k < 1) return ICV_OK;
    hipLaunchKernelGGL(icv::k_ward_pack_nn, dim3((unsigned)((k + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), w->mdesc + w->merged_begin(), w->h.n_pairs, w->act, w->h.n_act,
                       w->nn, w->dmin, w->map, d_nn, d_dmin);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_ward_unpack_nn(icv_ward_t w, const int32_t* d_nn, const float* d_dmin, void* stream) {
    if (!w || !d_nn || !d_dmin) return fail(ICV_ERR_INVALID, "bad ward_unpack_nn arguments");
    const int k = w->h.n_pairs + w->h.n_act;
    if (k < 1) return ICV_OK;
    hipLaunchKernelGGL(icv::k_ward_unpack_nn, dim3((unsigned)((k + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), w->mdesc + w->merged_begin(), w->h.n_pairs, w->act, w->h.n_act,
                       d_nn, d_dmin, w->nn, w->dmin);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_ward_pairs(icv_ward_t w, float* d_local, int64_t ld, int32_t all_active, int32_t* h_counts, void* stream) {
    if (!w || !h_counts || (!d_local && w->map.n_local > 0)) return fail(ICV_ERR_INVALID, "bad ward_pairs arguments");
    if (int rc = ward_check_ld(w, ld)) return rc;
    if (int rc = ward_pairs(w, d_local, ld, all_active != 0, static_cast<hipStream_t>(stream))) return rc;
    h_counts[0] = w->h.n_live;
    h_counts[1] = w->h.n_merges;
    h_counts[2] = w->h.n_pairs;
    h_counts[3] = w->h.n_act;
    return ICV_OK;
}

int icv_ward_round_pairs(icv_ward_t w, int32_t* h_i, int32_t* h_j) {
    if (!w || !h_i || !h_j) return fail(ICV_ERR_INVALID, "bad ward_round_pairs arguments");
    if (w->h.n_pairs < 1) return ICV_OK;
    HIP_TRY(hipMemcpy(h_i, w->log_i + w->merged_begin(), (size_t)w->h.n_pairs * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_j, w->log_j + w->merged_begin(), (size_t)w->h.n_pairs * 4, hipMemcpyDeviceToHost));
    return ICV_OK;
}

int icv_ward_finish(icv_ward_t w, double* h_linkage, int32_t* h_rounds) {
    if (!w || !h_linkage) return fail(ICV_ERR_INVALID, "bad ward_finish arguments");
    if (h_rounds) *h_rounds = w->rounds;
    return ward_finish(w, h_linkage);
}

int icv_row_abs_sum(const float* x, int64_t n_rows, int32_t n_cols, int64_t ld, double* row_sum, void* stream) {
    if (!x || !row_sum || n_cols < 0 || ld < n_cols) return fail(ICV_ERR_INVALID, "bad row_abs_sum arguments");
    if (n_rows < 1) return ICV_OK;
    hipLaunchKernelGGL(icv::k_row_abs_sum, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, n_rows, n_cols, ld, row_sum);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_csr_row_abs_sum(const void* data, int32_t dtype, const int64_t* indptr, int64_t n_rows, double* row_sum,
                        void* stream) {
    if (!indptr || !row_sum || (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad csr_row_abs_sum arguments");
    if (n_rows < 1) return ICV_OK;
    dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_csr_row_abs_sum<T>, grid, block, 0, st, static_cast<const T*>(data), indptr, n_rows, row_sum);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_csr_check(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_cols, int64_t capacity,
                  void* stream) {
    if (!indptr || n_rows < 0 || n_cols < 0 || capacity < 0 || (capacity > 0 && !indices))
        return fail(ICV_ERR_INVALID, "bad csr_check arguments");
    if (n_rows == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    AsyncBuf flag_b;
    HIP_TRY(flag_b.alloc(sizeof(int), st));
    HIP_TRY(hipMemsetAsync(flag_b.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(icv::k_csr_check, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, indptr, indices, n_rows,
                       n_cols, capacity, flag_b.as<int>());
    HIP_TRY(hipGetLastError());
    int h_flag = 0;
    HIP_TRY(hipMemcpyAsync(&h_flag, flag_b.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_flag & icv::kCsrBadOffsets)
        return fail(ICV_ERR_INVALID, "device CSR: row offsets must be non-decreasing and inside the index / value buffers");
    if (h_flag & icv::kCsrBadColumn) return fail(ICV_ERR_INVALID, "device CSR: a column index is outside [0, n_cols)");
    if (h_flag & icv::kCsrUnsorted)
        return fail(ICV_ERR_INVALID, "device CSR: column indices must be ascending and unique within every row "
                                     "(scipy: sum_duplicates() / sort_indices() before the upload)");
    return ICV_OK;
}

int icv_csr_densify(const void* data, int32_t dtype, const int64_t* indptr, const int32_t* indices, const int64_t* rows,
                    int64_t n_sel, int32_t n_cols, float* out, int64_t ldo, void* stream) {
    if (!indptr || !out || n_sel < 0 || n_cols < 0 || ldo < n_cols || (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad csr_densify arguments");
    if (n_sel == 0 || n_cols == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)((n_sel - 1) * ldo + n_cols) * sizeof(float), st));
    dim3 grid((unsigned)((n_sel + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_csr_densify<T>, grid, block, 0, st, static_cast<const T*>(data), indptr, indices, rows,
                           n_sel, out, ldo);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

static_assert(icv::kPcaKB == ICV_GRAM_BLOCK, "the header's block size is the kernel's");

int icv_gram_f64(const icv_matrix* m, int32_t panel_dtype, void* panel, int64_t panel_ld, double* g, int64_t ldg,
                 int32_t accumulate, void* stream) {
    if (!matrix_header_ok(m) || !g || m->n_cols < 1 || ldg < m->n_cols || (panel_dtype != ICV_F32 && panel_dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad gram_f64 arguments");
    const int n = m->n_cols, n_t = (n + icv::kPcaT - 1) / icv::kPcaT, n_tri = n_t * (n_t + 1) / 2;
    if (m->n_rows > 0 && (!panel || panel_ld < (int64_t)n_t * icv::kPcaT))
        return fail(ICV_ERR_INVALID, "gram_f64: the panel needs a row stride of at least n_cols rounded up to 64");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m->n_rows == 0) {
        if (!accumulate) hipLaunchKernelGGL(icv::k_gram_reduce, dim3((unsigned)n_tri), dim3(256), 0, st, nullptr, 0, n_t,
                                            n, g, ldg, 0);
        HIP_TRY(hipGetLastError());
        return ICV_OK;
    }
    const int64_t rows = m->n_rows, n_pad = (rows + icv::kPcaKC - 1) / icv::kPcaKC * icv::kPcaKC;
    const size_t esz = panel_dtype == ICV_F32 ? 4 : 8;
    HIP_TRY(hipMemsetAsync(panel, 0, (size_t)n_pad * panel_ld * esz, st));
    const dim3 rgrid((unsigned)((rows + 3) / 4)), rblock(256);
    by_matrix(m, [&](auto t, auto csr) {
        by_dtype(panel_dtype, [&](auto p) {
            using T = decltype(t);
            using P = decltype(p);
            if constexpr (decltype(csr)::value)
                hipLaunchKernelGGL((icv::k_pca_panel_csr<T, P>), rgrid, rblock, 0, st, (const T*)m->values, m->indptr,
                                   m->indices, rows, (P*)panel, panel_ld);
            else
                hipLaunchKernelGGL((icv::k_pca_panel_dense<T, P>), rgrid, rblock, 0, st, (const T*)m->values, m->ld, rows, n,
                                   (P*)panel, panel_ld);
        });
    });
    HIP_TRY(hipGetLastError());
    // partial tiles of up to 256 MB per launch pair; the reduction adds them to G in block order either way
    const int64_t n_blocks = (n_pad + icv::kPcaKB - 1) / icv::kPcaKB;
    const size_t tile_bytes = (size_t)n_tri * icv::kPcaT * icv::kPcaT * sizeof(double);
    int64_t per = (int64_t)((256ull << 20) / tile_bytes);
    per = per < 1 ? 1 : (per > n_blocks ? n_blocks : per);
    AsyncBuf part_b;
    HIP_TRY(part_b.alloc((size_t)per * tile_bytes, st));
    for (int64_t b0 = 0; b0 < n_blocks; b0 += per) {
        const int64_t nb = per < n_blocks - b0 ? per : n_blocks - b0;
        const int64_t c0 = b0 * icv::kPcaKB;
        const int64_t np = n_pad - c0 < nb * icv::kPcaKB ? n_pad - c0 : nb * icv::kPcaKB;
        const dim3 grid((unsigned)n_tri, (unsigned)nb);
        by_dtype(panel_dtype, [&](auto p) {
            using P = decltype(p);
            hipLaunchKernelGGL(icv::k_gram_f64<P>, grid, dim3(256), 0, st, (const P*)panel + c0 * panel_ld, panel_ld, np,
                               n_t, part_b.as<double>());
        });
        hipLaunchKernelGGL(icv::k_gram_reduce, dim3((unsigned)n_tri), dim3(256), 0, st, part_b.as<double>(), (int)nb,
                           n_t, n, g, ldg, (accumulate || b0 > 0) ? 1 : 0);
    }
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_project(const icv_matrix* m, const double* v, int32_t k, const double* shift, int32_t out_dtype, void* out,
                int64_t ldo, void* stream) {
    if (!matrix_header_ok(m) || !v || !out || k < 1 || ldo < k || (out_dtype != ICV_F32 && out_dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad project arguments");
    if (m->n_rows == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((m->n_rows + 3) / 4)), block(256);
    by_matrix(m, [&](auto t, auto csr) {
        by_dtype(out_dtype, [&](auto o) {
            using T = decltype(t);
            using O = decltype(o);
            if constexpr (decltype(csr)::value)
                hipLaunchKernelGGL((icv::k_csr_project<T, O>), grid, block, 0, st, (const T*)m->values, m->indptr, m->indices,
                                   m->n_rows, v, k, shift, (O*)out, ldo);
            else
                hipLaunchKernelGGL((icv::k_dense_project<T, O>), grid, block, 0, st, (const T*)m->values, m->ld, m->n_rows,
                                   m->n_cols, v, k, shift, (O*)out, ldo);
        });
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // extern "C"

// ---- host-side packing of a mostly-zero dense matrix (the upload path of tl.infercnv for dense host input) ---------------
namespace {
template <typename T>
using host_bits = std::conditional_t<sizeof(T) == 4, uint32_t, uint64_t>;  // an element's bit pattern

template <typename T, typename B>
void host_count_rows(const T* x, int64_t r0, int64_t r1, int64_t n_cols, int64_t ld, int64_t* row_nnz) {
    for (int64_t r = r0; r < r1; ++r) {
        const B* b = reinterpret_cast<const B*>(x + r * ld);
        int64_t c = 0;
        for (int64_t j = 0; j < n_cols; ++j) c += b[j] != 0;  // bit pattern: NaN and -0.0 are stored entries
        row_nnz[r] = c;
    }
}
// elements [j, n_cols) of one row, entries from cursor k on (k < end while there is something to find): branch-free,
// every element is written at the cursor and the cursor moves on for stored ones; never writes at or past `end`
template <typename T, typename B>
inline void host_pack_tail(const T* xr, int64_t j, int64_t n_cols, int64_t k, int64_t end, int32_t* indices, T* values) {
    const B* b = reinterpret_cast<const B*>(xr);
    for (; j < n_cols && k < end; ++j) {
        indices[k] = (int32_t)j;
        values[k] = xr[j];
        k += b[j] != 0;
    }
}
template <typename T, typename B>
void host_pack_rows(const T* x, int64_t r0, int64_t r1, int64_t n_cols, int64_t ld, const int64_t* indptr,
                    int32_t* indices, T* values) {
    for (int64_t r = r0; r < r1; ++r) {
        const T* xr = x + r * ld;
        const int64_t k = indptr[r], end = indptr[r + 1];
        if (end - k == n_cols) {  // a full row: no test per element
            for (int64_t j = 0; j < n_cols; ++j) indices[k + j] = (int32_t)j, values[k + j] = xr[j];
            continue;
        }
        host_pack_tail<T, B>(xr, 0, n_cols, k, end, indices, values);
    }
}

// AVX-512 forms (chosen at run time: the library is built on one machine and runs on another).  Register compress +
// full-width store (the memory-destination compress is microcoded on some cores); a vector is only stored while 16 (8)
// slots of THIS row are left, the last entries of a row go through the scalar tail -- nothing is written outside
// [indptr[r], indptr[r + 1]), so rows can be packed by different threads.
#if defined(__x86_64__)
__attribute__((target("avx512f,avx512vl,avx512bw,popcnt")))
void host_count_rows_avx512(const float* x, int64_t r0, int64_t r1, int64_t n_cols, int64_t ld, int64_t* row_nnz) {
    for (int64_t r = r0; r < r1; ++r) {
        const float* xr = x + r * ld;
        int64_t c = 0, j = 0;
        for (; j + 16 <= n_cols; j += 16) {
            const __m512i v = _mm512_loadu_si512((const void*)(xr + j));
            c += _mm_popcnt_u32((unsigned)_mm512_test_epi32_mask(v, v));
        }
        const uint32_t* b = reinterpret_cast<const uint32_t*>(xr);
        for (; j < n_cols; ++j) c += b[j] != 0;
        row_nnz[r] = c;
    }
}
__attribute__((target("avx512f,avx512vl,avx512bw,popcnt")))
void host_count_rows_avx512(const double* x, int64_t r0, int64_t r1, int64_t n_cols, int64_t ld, int64_t* row_nnz) {
    for (int64_t r = r0; r < r1; ++r) {
        const double* xr = x + r * ld;
        int64_t c = 0, j = 0;
        for (; j + 8 <= n_cols; j += 8) {
            const __m512i v = _mm512_loadu_si512((const void*)(xr + j));
            c += _mm_popcnt_u32((unsigned)_mm512_test_epi64_mask(v, v));
        }
        const uint64_t* b = reinterpret_cast<const uint64_t*>(xr);
        for (; j < n_cols; ++j) c += b[j] != 0;
        row_nnz[r] = c;
    }
}
__attribute__((target("avx512f,avx512vl,avx512bw,popcnt")))
void host_pack_rows_avx512(const float* x, int64_t r0, int64_t r1, int64_t n_cols, int64_t ld, const int64_t* indptr,
                               int32_t* indices, float* values) {
    const __m512i iota = _mm512_setr_epi32(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    for (int64_t r = r0; r < r1; ++r) {
        const float* xr = x + r * ld;
        int64_t k = indptr[r];
        const int64_t end = indptr[r + 1];
        int64_t j = 0;
        for (; j + 16 <= n_cols && k + 16 <= end; j += 16) {
            const __m512i v = _mm512_loadu_si512((const void*)(xr + j));
            const __mmask16 m = _mm512_test_epi32_mask(v, v);
            _mm512_storeu_si512((void*)(values + k), _mm512_maskz_compress_epi32(m, v));
            _mm512_storeu_si512((void*)(indices + k),
                                _mm512_maskz_compress_epi32(m, _mm512_add_epi32(iota, _mm512_set1_epi32((int)j))));
            k += _mm_popcnt_u32((unsigned)m);
        }
        host_pack_tail<float, uint32_t>(xr, j, n_cols, k, end, indices, values);
    }
}
__attribute__((target("avx512f,avx512vl,avx512bw,popcnt")))
void host_pack_rows_avx512(const double* x, int64_t r0, int64_t r1, int64_t n_cols, int64_t ld, const int64_t* indptr,
                               int32_t* indices, double* values) {
    const __m256i iota = _mm256_setr_epi32(0, 1, 2, 3, 4, 5, 6, 7);
    for (int64_t r = r0; r < r1; ++r) {
        const double* xr = x + r * ld;
        int64_t k = indptr[r];
        const int64_t end = indptr[r + 1];
        int64_t j = 0;
        for (; j + 8 <= n_cols && k + 8 <= end; j += 8) {
            const __m512i v = _mm512_loadu_si512((const void*)(xr + j));
            const __mmask8 m = _mm512_test_epi64_mask(v, v);
            _mm512_storeu_si512((void*)(values + k), _mm512_maskz_compress_epi64(m, v));
            _mm256_storeu_si256((__m256i*)(indices + k),
                                _mm256_maskz_compress_epi32(m, _mm256_add_epi32(iota, _mm256_set1_epi32((int)j))));
            k += _mm_popcnt_u32((unsigned)m);
        }
        host_pack_tail<double, uint64_t>(xr, j, n_cols, k, end, indices, values);
    }
}
// one row into a staging area with 16 slots of slack behind the row's worst case: no bound to respect, returns the count
__attribute__((target("avx512f,avx512vl,avx512bw,popcnt")))
int64_t host_pack_row_avx512(const float* xr, int64_t n_cols, int32_t* indices, float* values) {
    const __m512i iota = _mm512_setr_epi32(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    int64_t k = 0, j = 0;
    for (; j + 16 <= n_cols; j += 16) {
        const __m512i v = _mm512_loadu_si512((const void*)(xr + j));
        const __mmask16 m = _mm512_test_epi32_mask(v, v);
        _mm512_storeu_si512((void*)(values + k), _mm512_maskz_compress_epi32(m, v));
        _mm512_storeu_si512((void*)(indices + k),
                            _mm512_maskz_compress_epi32(m, _mm512_add_epi32(iota, _mm512_set1_epi32((int)j))));
        k += _mm_popcnt_u32((unsigned)m);
    }
    const uint32_t* b = reinterpret_cast<const uint32_t*>(xr);
    for (; j < n_cols; ++j) {
        indices[k] = (int32_t)j;
        values[k] = xr[j];
        k += b[j] != 0;
    }
    return k;
}
__attribute__((target("avx512f,avx512vl,avx512bw,popcnt")))
int64_t host_pack_row_avx512(const double* xr, int64_t n_cols, int32_t* indices, double* values) {
    const __m256i iota = _mm256_setr_epi32(0, 1, 2, 3, 4, 5, 6, 7);
    int64_t k = 0, j = 0;
    for (; j + 8 <= n_cols; j += 8) {
        const __m512i v = _mm512_loadu_si512((const void*)(xr + j));
        const __mmask8 m = _mm512_test_epi64_mask(v, v);
        _mm512_storeu_si512((void*)(values + k), _mm512_maskz_compress_epi64(m, v));
        _mm256_storeu_si256((__m256i*)(indices + k),
                            _mm256_maskz_compress_epi32(m, _mm256_add_epi32(iota, _mm256_set1_epi32((int)j))));
        k += _mm_popcnt_u32((unsigned)m);
    }
    const uint64_t* b = reinterpret_cast<const uint64_t*>(xr);
    for (; j < n_cols; ++j) {
        indices[k] = (int32_t)j;
        values[k] = xr[j];
        k += b[j] != 0;
    }
    return k;
}
bool host_has_avx512() {
    static const bool ok = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512vl") &&
                           __builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("popcnt") &&
                           std::getenv("ICV_NO_AVX512") == nullptr;
    return ok;
}
#else
bool host_has_avx512() { return false; }
#endif
template <typename T, typename B>
int64_t host_pack_row_scalar(const T* xr, int64_t n_cols, int32_t* indices, T* values) {
    const B* b = reinterpret_cast<const B*>(xr);
    int64_t k = 0;
    for (int64_t j = 0; j < n_cols; ++j) {
        indices[k] = (int32_t)j;
        values[k] = xr[j];
        k += b[j] != 0;
    }
    return k;
}

// ONE pass over the input: threads claim blocks of kFusedRows rows in order, pack a block into their own staging area
// (cache resident at log-count densities), take the block's place in the output through a ticket that is handed on in
// block order (a running entry count), and copy the block there.  The input is read once; the two-pass form (count,
// prefix sums, pack) reads it twice, and the host memory system is what the upload of a 16 GB matrix waits for.
constexpr int64_t kFusedRows = 16;

// Staging areas of the packing threads, kept between calls: 128 threads that each map (and fault in) 2.5 MB per call
// serialise on the process's address-space lock -- the first version of the one-pass form was slower with 128 threads
// (0.6 - 1.7 s per 16 GB) than with 32 (0.23 - 0.35 s).
struct HostStagePool {
    std::mutex mu;
    std::vector<std::pair<unsigned char*, size_t>> idle;
    size_t idle_bytes = 0;
    unsigned char* take(size_t bytes, size_t* got) {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < idle.size(); ++i)
                if (idle[i].second >= bytes) {
                    unsigned char* p = idle[i].first;
                    *got = idle[i].second;
                    idle_bytes -= idle[i].second;
                    idle[i] = idle.back();
                    idle.pop_back();
                    return p;
                }
        }
        *got = bytes;
        return static_cast<unsigned char*>(std::malloc(bytes));
    }
    void give(unsigned char* p, size_t bytes) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (idle_bytes + bytes <= (size_t)1 << 30 && idle.size() < 512) {
                idle.emplace_back(p, bytes);
                idle_bytes += bytes;
                return;
            }
        }
        std::free(p);
    }
};
HostStagePool g_stage_pool;

template <typename T, typename B>
int host_pack_fused(const T* x, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t* indptr, int32_t* indices, T* values,
                    int64_t capacity, int n_threads, int64_t* total_out) {
    const int64_t n_blocks = (n_rows + kFusedRows - 1) / kFusedRows;
    if (n_threads < 1) n_threads = 1;
    if ((int64_t)n_threads > n_blocks) n_threads = (int)(n_blocks > 0 ? n_blocks : 1);
    std::atomic<int64_t> next_claim{0}, next_commit{0};
    int64_t total = 0;  // written by the ticket holder only
    std::atomic<bool> overflow{false}, failed{false};
    const bool vec = host_has_avx512();
    indptr[0] = 0;
    auto worker = [&]() {
        const size_t cap = (size_t)kFusedRows * (size_t)n_cols + 32;
        size_t got = 0;
        unsigned char* raw = g_stage_pool.take(cap * (sizeof(int32_t) + sizeof(T)) + 64, &got);
        if (!raw) {
            overflow.store(true);  // (reported as out of memory by the caller; the tickets below must still be passed on)
            failed.store(true);
        }
        struct Give {
            unsigned char* p;
            size_t n;
            ~Give() { g_stage_pool.give(p, n); }
        } give_back{raw, got};
        T* s_val_p = reinterpret_cast<T*>(raw);  // (values first: 8-byte aligned)
        int32_t* s_idx_p = reinterpret_cast<int32_t*>(raw + cap * sizeof(T));
        int64_t cnt[kFusedRows];
        for (;;) {
            const int64_t k = next_claim.fetch_add(1, std::memory_order_relaxed);
            if (k >= n_blocks) return;
            const int64_t r0 = k * kFusedRows, r1 = r0 + kFusedRows < n_rows ? r0 + kFusedRows : n_rows;
            int64_t n = 0;
            for (int64_t r = r0; r < r1 && raw; ++r) {
                const T* xr = x + r * ld;
                int64_t c;
#if defined(__x86_64__)
                if (vec) {
                    c = host_pack_row_avx512(xr, n_cols, s_idx_p + n, s_val_p + n);
                } else
#endif
                    c = host_pack_row_scalar<T, B>(xr, n_cols, s_idx_p + n, s_val_p + n);
                cnt[r - r0] = c;
                n += c;
            }
            if (!raw)
                for (int64_t r = r0; r < r1; ++r) cnt[r - r0] = 0;
            // the ticket: blocks take their place in block order (a few loads, then the thread steps aside -- 128
            // threads spinning on one cache line slow down the one that has to write it)
            for (int spins = 0; next_commit.load(std::memory_order_acquire) != k; ++spins) {
                if (spins < 64) {
#if defined(__x86_64__)
                    _mm_pause();
#endif
                } else {
                    std::this_thread::yield();
                }
            }
            const int64_t off = total;
            total = off + n;
            int64_t run = off;
            for (int64_t r = r0; r < r1; ++r) {
                run += cnt[r - r0];
                indptr[r + 1] = run;
            }
            const bool fits = off + n <= capacity;
            if (!fits) overflow.store(true, std::memory_order_relaxed);
            next_commit.store(k + 1, std::memory_order_release);
            if (fits && n) {
                std::memcpy(indices + off, s_idx_p, (size_t)n * sizeof(int32_t));
                std::memcpy(values + off, s_val_p, (size_t)n * sizeof(T));
            }
        }
    };
    if (n_threads == 1) {
        worker();
    } else {
        // (a thread that cannot be created -- ulimit, exhaustion -- must not leave joinable threads behind: the blocks are
        // claimed by whoever runs, so the threads that did start, and this one, finish the piece: ADVICE r5)
        std::vector<std::thread> pool;
        pool.reserve(n_threads);
        bool short_of_threads = false;
        for (int t = 0; t < n_threads && !short_of_threads; ++t) {
            try {
                pool.emplace_back(worker);
            } catch (const std::system_error&) {
                short_of_threads = true;
            }
        }
        if (short_of_threads) worker();
        for (auto& th : pool) th.join();
    }
    *total_out = total;
    if (failed.load()) throw std::bad_alloc();
    return overflow.load() ? 1 : 0;
}

template <typename F>
void host_parallel_rows(int64_t n_rows, int n_threads, F&& fn) {
    if (n_threads < 1) n_threads = 1;
    if ((int64_t)n_threads > n_rows) n_threads = (int)(n_rows > 0 ? n_rows : 1);
    if (n_threads == 1) {
        fn((int64_t)0, n_rows);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve(n_threads);
    for (int t = 0; t < n_threads; ++t) {
        const int64_t a = n_rows * t / n_threads, b = n_rows * (t + 1) / n_threads;
        try {
            pool.emplace_back([&fn, a, b] { fn(a, b); });
        } catch (const std::system_error&) {
            fn(a, b);  // no thread to be had: this range on the calling thread
        }
    }
    for (auto& th : pool) th.join();
}
}  // namespace

extern "C" {

int icv_host_dense_row_nnz(const void* h_x, int32_t dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                           int64_t* h_row_nnz, int32_t n_threads) {
    if (!h_x || !h_row_nnz || n_rows < 0 || n_cols < 0 || ld < n_cols || (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad host_dense_row_nnz arguments");
    try {
        const bool vec = host_has_avx512();
        by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            host_parallel_rows(n_rows, n_threads, [&](int64_t a, int64_t b) {
#if defined(__x86_64__)
                if (vec) return host_count_rows_avx512((const T*)h_x, a, b, n_cols, ld, h_row_nnz);
#endif
                host_count_rows<T, host_bits<T>>((const T*)h_x, a, b, n_cols, ld, h_row_nnz);
            });
        });
    } catch (const std::exception& e) {
        return fail(ICV_ERR_NOMEM, std::string("host_dense_row_nnz: ") + e.what());
    }
    return ICV_OK;
}

int icv_host_dense_pack(const void* h_x, int32_t dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                        const int64_t* h_indptr, int32_t* h_indices, void* h_values, int32_t n_threads) {
    if (!h_x || !h_indptr || !h_indices || !h_values || n_rows < 0 || n_cols < 0 || ld < n_cols ||
        (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad host_dense_pack arguments");
    try {
        const bool vec = host_has_avx512();
        by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            host_parallel_rows(n_rows, n_threads, [&](int64_t a, int64_t b) {
#if defined(__x86_64__)
                if (vec) return host_pack_rows_avx512((const T*)h_x, a, b, n_cols, ld, h_indptr, h_indices, (T*)h_values);
#endif
                host_pack_rows<T, host_bits<T>>((const T*)h_x, a, b, n_cols, ld, h_indptr, h_indices, (T*)h_values);
            });
        });
    } catch (const std::exception& e) {
        return fail(ICV_ERR_NOMEM, std::string("host_dense_pack: ") + e.what());
    }
    return ICV_OK;
}

int icv_host_dense_pack_fused(const void* h_x, int32_t dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                              int64_t* h_indptr, int32_t* h_indices, void* h_values, int64_t capacity,
                              int32_t n_threads, int64_t* h_nnz) {
    if (!h_x || !h_indptr || !h_nnz || n_rows < 0 || n_cols < 0 || ld < n_cols || capacity < 0 ||
        (capacity > 0 && (!h_indices || !h_values)) || (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad host_dense_pack_fused arguments");
    try {
        const int over = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return host_pack_fused<T, host_bits<T>>((const T*)h_x, n_rows, n_cols, ld, h_indptr, h_indices, (T*)h_values,
                                                    capacity, n_threads, h_nnz);
        });
        if (over)
            return fail(ICV_ERR_NOMEM, "host_dense_pack_fused: the matrix holds more stored entries than `capacity` "
                                       "(*h_nnz has the count: call again with larger buffers)");
    } catch (const std::exception& e) {
        return fail(ICV_ERR_NOMEM, std::string("host_dense_pack_fused: ") + e.what());
    }
    return ICV_OK;
}

int icv_csr_scatter_dense(const void* data, int32_t dtype, const int64_t* indptr, const int32_t* indices, int64_t n_rows,
                          int32_t n_cols, void* out, int64_t ldo, void* stream) {
    if (!indptr || !out || n_rows < 0 || n_cols < 0 || ldo < n_cols || (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad csr_scatter_dense arguments");
    if (n_rows == 0 || n_cols == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t esz = dtype == ICV_F32 ? 4 : 8;
    if (ldo == n_cols)
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_rows * n_cols * esz, st));
    else
        HIP_TRY(hipMemset2DAsync(out, (size_t)ldo * esz, 0, (size_t)n_cols * esz, (size_t)n_rows, st));
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_csr_scatter_rows<T>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st,
                           static_cast<const T*>(data), indptr, indices, n_rows, static_cast<T*>(out), ldo);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_group_sums(const double* values, const int32_t* group, int64_t n, int32_t n_groups, double* sums,
                   int64_t* counts, void* stream) {
    if (!sums || !counts || n < 0 || n_groups < 0 || (n > 0 && (!values || !group)))
        return fail(ICV_ERR_INVALID, "bad group_sums arguments");
    if (n_groups == 0) return ICV_OK;
    hipLaunchKernelGGL(icv::k_group_sums, dim3((unsigned)n_groups), dim3(1024), 0, static_cast<hipStream_t>(stream),
                       values, group, n, sums, counts);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // extern "C"

// ---- what pp.neighbors, tl.leiden, tl.umap and tl.tsne share ---------------------------------------------------------
namespace {
#define ICV_TRY(expr)              \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_ != ICV_OK) return rc_; \
    } while (0)

inline dim3 ld_grid(int64_t n, int per = 256) { return dim3((unsigned)((n + per - 1) / per)); }

// a workspace laid out as segments of whole 256-byte units: seg(b) is the offset of the next one, seg.o the total
struct Seg {
    size_t o = 0;
    size_t operator()(size_t b) {
        const size_t at = o;
        o += (b + 255) / 256 * 256;
        return at;
    }
};

// The event pair behind stage_ms (nothing is created or recorded without it): toc(slot) waits for the stage and adds
// its milliseconds to ms[slot], which for a slot that is timed once is the stage's time itself.
struct StageTimer {
    hipStream_t st;
    bool on;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float ms[4] = {0, 0, 0, 0};
    StageTimer(hipStream_t s, const float* stage_ms) : st(s), on(stage_ms != nullptr) {}
    ~StageTimer() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    hipError_t create() {
        if (!on) return hipSuccess;
        const hipError_t e = hipEventCreate(&ev0);
        return e != hipSuccess ? e : hipEventCreate(&ev1);
    }
    hipError_t tic() { return on ? hipEventRecord(ev0, st) : hipSuccess; }
    hipError_t toc(int slot) {
        if (!on) return hipSuccess;
        hipError_t e = hipEventRecord(ev1, st);
        if (e != hipSuccess) return e;
        e = hipEventSynchronize(ev1);
        if (e != hipSuccess) return e;
        float t = 0;
        e = hipEventElapsedTime(&t, ev0, ev1);
        ms[slot] += t;
        return e;
    }
};

bool graph_sizes_ok(int64_t n, int64_t nnz) { return n >= 1 && n <= (int64_t)1 << 30 && nnz >= 0 && nnz < (int64_t)1 << 31; }
bool components_ok(int32_t c) { return c == 2 || c == 3; }

// the report of the flags of icv::graph_entry_flags, in the order they are tested; ICV_OK without one
int graph_flags_error(const char* who, unsigned f) {
    const char* what = f & 8    ? "the adjacency matrix has a column index out of range"
                       : f & 16 ? "the rows of the adjacency matrix must be sorted, without duplicates"
                       : f & 1  ? "the adjacency matrix has non-finite values"
                       : f & 2  ? "the adjacency matrix has negative values"
                       : f & 4  ? "the adjacency matrix has stored diagonal entries"
                       : f & 32 ? "the adjacency matrix is not symmetric"
                                : nullptr;
    return what ? fail(ICV_ERR_INVALID, std::string(who) + ": " + what) : ICV_OK;
}

// k_graph_check on the float32 graph and its four words, read back (head: 16 bytes of the workspace or more)
struct GraphCheck {
    unsigned flags, n_long;
    float w_max;      // largest finite non-negative weight
    int64_t longest;  // entries of the longest row
};
int run_graph_check(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, unsigned* head,
                    int32_t* long_list, hipStream_t st, GraphCheck* out) {
    HIP_TRY(hipMemsetAsync(head, 0, 16, st));
    hipLaunchKernelGGL(icv::k_graph_check, ld_grid(n, 4), dim3(256), 0, st, indptr, indices, data, n, head, long_list);
    HIP_TRY(hipGetLastError());
    unsigned h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, head, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->flags = h[0], out->n_long = h[1], out->longest = (int64_t)h[3];
    std::memcpy(&out->w_max, &h[2], 4);
    return ICV_OK;
}

// A + A^T (SUM) or A + A^T - A o A^T of `per_row` neighbours per row: the row lengths, then the canonical CSR
template <bool SUM>
int symmetrize_count(const int32_t* knn_idx, const double* w, int64_t n, int per_row, int64_t* row_nnz, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(row_nnz, 0, (size_t)n * sizeof(int64_t), st));
    hipLaunchKernelGGL(icv::k_knn_sym_count<SUM>, ld_grid(n * per_row), dim3(256), 0, st, knn_idx, w, n, per_row,
                       reinterpret_cast<unsigned long long*>(row_nnz));
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}
template <bool SUM>
int symmetrize_fill(const int32_t* knn_idx, const double* w, int64_t n, int per_row, const int64_t* indptr, int64_t nnz,
                    int32_t* indices, float* data, hipStream_t st) {
    AsyncBuf cur, tc, tv;
    HIP_TRY(cur.alloc((size_t)n * sizeof(unsigned), st));
    HIP_TRY(tc.alloc((size_t)nnz * sizeof(int32_t), st));
    HIP_TRY(tv.alloc((size_t)nnz * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(cur.p, 0, (size_t)n * sizeof(unsigned), st));
    hipLaunchKernelGGL(icv::k_knn_sym_fill<SUM>, ld_grid(n * per_row), dim3(256), 0, st, knn_idx, w, n, per_row, indptr,
                       cur.as<unsigned>(), tc.as<int32_t>(), tv.as<float>());
    hipLaunchKernelGGL(icv::k_knn_sort_rows, ld_grid(n, 4), dim3(256), 0, st, indptr, n, tc.as<int32_t>(), tv.as<float>(),
                       indices, data);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}
}  // namespace

// ---- pp.neighbors (csrc/icv_knn.hpp) ---------------------------------------------------------------------------------
namespace {
struct KnnGeom {
    int dp, nk, L, parts, n_slabs;
    int64_t n_pad, chunk, rows_per;
    size_t off_partial, off_mu, off_flags, off_z, off_snorm, off_cand, off_bound, off_redo, bytes;
    KnnGeom(int64_t n, int d, int k) {
        dp = d <= 64 ? 64 : d <= 128 ? 128 : 256;
        nk = dp / 8;
        L = k - 1 + icv::kKnnSlack;
        n_pad = (n + icv::kKnnRows - 1) / icv::kKnnRows * icv::kKnnRows;
        const int64_t gx = n_pad / icv::kKnnRows;
        int64_t want = 2048 / gx;
        want = want < 1 ? 1 : want > icv::kKnnMaxParts ? icv::kKnnMaxParts : want;
        chunk = ((n_pad + want - 1) / want + 31) / 32 * 32;
        parts = (int)((n_pad + chunk - 1) / chunk);
        rows_per = (n + 1023) / 1024;
        if (rows_per < 64) rows_per = 64;
        n_slabs = (int)((n + rows_per - 1) / rows_per);
        Seg seg;
        off_partial = seg((size_t)n_slabs * d * 8);
        off_mu = seg(256 * 4);
        off_flags = seg(16);
        off_z = seg((size_t)n_pad * dp * 4);
        off_snorm = seg((size_t)n_pad * 4);
        off_cand = seg((size_t)n * parts * 2 * L * 4);
        off_bound = seg((size_t)n * parts * 2 * 4);
        off_redo = seg((size_t)n * 4);
        bytes = seg.o;
    }
};
int knn_args_ok(int64_t n, int32_t d, int32_t k) {
    return n >= 2 && n <= (int64_t)1 << 30 && d >= 1 && d <= 256 && k >= 2 && k <= 64 && k <= n;
}
}  // namespace

extern "C" {

int icv_knn_workspace(int64_t n, int32_t d, int32_t k, int64_t* bytes) {
    if (!bytes || !knn_args_ok(n, d, k)) return fail(ICV_ERR_INVALID, "bad knn_workspace arguments");
    *bytes = (int64_t)KnnGeom(n, d, k).bytes;
    return ICV_OK;
}

int icv_knn(const float* x, int64_t n, int32_t d, int64_t ld, int32_t k, void* workspace, int32_t* knn_idx,
            float* knn_dist, int32_t* n_exact, float* stage_ms, void* stream) {
    if (!x || !workspace || !knn_idx || !knn_dist || !knn_args_ok(n, d, k) || ld < d)
        return fail(ICV_ERR_INVALID, "bad knn arguments (2 <= k <= min(n, 64), 1 <= d <= 256)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const KnnGeom G(n, d, k);
    char* ws = static_cast<char*>(workspace);
    double* partial = reinterpret_cast<double*>(ws + G.off_partial);
    float* mu = reinterpret_cast<float*>(ws + G.off_mu);
    unsigned* maxbits = reinterpret_cast<unsigned*>(ws + G.off_flags);
    unsigned* n_redo = maxbits + 1;
    float* z = reinterpret_cast<float*>(ws + G.off_z);
    float* snorm = reinterpret_cast<float*>(ws + G.off_snorm);
    int32_t* cand = reinterpret_cast<int32_t*>(ws + G.off_cand);
    float* bound = reinterpret_cast<float*>(ws + G.off_bound);
    int32_t* redo = reinterpret_cast<int32_t*>(ws + G.off_redo);
    const int km1 = k - 1;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 5; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } ev_guard{ev};
    auto mark = [&](int i) -> hipError_t {
        if (!stage_ms) return hipSuccess;
        hipError_t e = hipEventCreate(&ev[i]);
        return e != hipSuccess ? e : hipEventRecord(ev[i], st);
    };

    HIP_TRY(mark(0));
    hipLaunchKernelGGL(icv::k_knn_colsum, dim3((unsigned)G.n_slabs), dim3(256), 0, st, x, n, d, ld, G.rows_per, partial);
    hipLaunchKernelGGL(icv::k_knn_mean, dim3(1), dim3(256), 0, st, partial, G.n_slabs, d, n, mu, maxbits);
    const double cfac = (double)(G.dp + 16) * 5.9604644775390625e-08;  // (DP + 16) 2^-24
    hipLaunchKernelGGL(icv::k_knn_center, dim3((unsigned)(G.n_pad / 256 + 1)), dim3(256), 0, st, x, n, G.n_pad, d, ld, G.dp,
                       mu, cfac, z, snorm, maxbits);
    HIP_TRY(hipMemsetAsync(n_redo, 0, sizeof(unsigned), st));
    HIP_TRY(mark(1));
    const size_t lds = (size_t)4 * 2 * G.L * 64 * 4;
    const dim3 grid((unsigned)(G.n_pad / icv::kKnnRows), (unsigned)G.parts);
#define ICV_KNN_SWEEP(NK)                                                                                              \
    {                                                                                                                  \
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(icv::k_knn_candidates<NK>),                          \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                            \
        hipLaunchKernelGGL(icv::k_knn_candidates<NK>, grid, dim3(256), lds, st, z, snorm, n, G.n_pad, G.chunk, G.L,    \
                           cand, bound);                                                                               \
    }
    if (G.nk == 8) ICV_KNN_SWEEP(8)
    else if (G.nk == 16) ICV_KNN_SWEEP(16)
    else ICV_KNN_SWEEP(32)
#undef ICV_KNN_SWEEP
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(2));
    const size_t lds_r = (size_t)G.parts * 2 * G.L * 12;
    hipLaunchKernelGGL(icv::k_knn_rerank, dim3((unsigned)n), dim3(64), lds_r, st, x, n, d, ld, cand, bound, G.parts, G.L,
                       km1, maxbits, knn_idx, knn_dist, redo, n_redo);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(3));
    unsigned h_redo = 0;
    HIP_TRY(hipMemcpyAsync(&h_redo, n_redo, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_redo > 0) {
        hipLaunchKernelGGL(icv::k_knn_exact, dim3(h_redo), dim3(256), 0, st, x, n, d, ld, km1, redo, knn_idx, knn_dist);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(mark(4));
    if (n_exact) *n_exact = (int32_t)h_redo;
    if (stage_ms) {
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(stage_ms + i, ev[i], ev[i + 1]));
    }
    return ICV_OK;
}

int icv_knn_fuzzy(const float* knn_dist, int64_t n, int32_t k, double* rho, double* sigma, double* weights, void* stream) {
    if (!knn_dist || !rho || !sigma || !weights || n < 1 || k < 2 || k > 64)
        return fail(ICV_ERR_INVALID, "bad knn_fuzzy arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AsyncBuf tmp;
    HIP_TRY(tmp.alloc((size_t)(n + 1) * sizeof(double), st));
    double* rowsum = tmp.as<double>();
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(icv::k_knn_rowsum, grid, dim3(256), 0, st, knn_dist, n, k - 1, rowsum);
    hipLaunchKernelGGL(icv::k_knn_total, dim3(1), dim3(1024), 0, st, rowsum, n, rowsum + n);
    hipLaunchKernelGGL(icv::k_knn_smooth, grid, dim3(256), 0, st, knn_dist, n, k - 1, rowsum, rowsum + n, rho, sigma, weights);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_knn_symmetrize_count(const int32_t* knn_idx, const double* weights, int64_t n, int32_t k, int64_t* row_nnz,
                             void* stream) {
    if (!knn_idx || !weights || !row_nnz || n < 1 || k < 2 || k > 64)
        return fail(ICV_ERR_INVALID, "bad knn_symmetrize_count arguments");
    return symmetrize_count<false>(knn_idx, weights, n, k - 1, row_nnz, static_cast<hipStream_t>(stream));
}

int icv_knn_symmetrize_fill(const int32_t* knn_idx, const double* weights, int64_t n, int32_t k, const int64_t* indptr,
                            int64_t nnz, int32_t* indices, float* data, void* stream) {
    if (!knn_idx || !weights || !indptr || !indices || !data || n < 1 || k < 2 || k > 64 || nnz < 0 ||
        nnz > 2 * n * (int64_t)(k - 1))
        return fail(ICV_ERR_INVALID, "bad knn_symmetrize_fill arguments");
    return symmetrize_fill<false>(knn_idx, weights, n, k - 1, indptr, nnz, indices, data, static_cast<hipStream_t>(stream));
}

int icv_knn_sort_rows(const int64_t* indptr, int64_t n, const int32_t* cols_in, const float* vals_in, int32_t* cols,
                      float* vals, void* stream) {
    if (!indptr || !cols_in || !vals_in || !cols || !vals || n < 1 || cols_in == cols || vals_in == vals)
        return fail(ICV_ERR_INVALID, "bad knn_sort_rows arguments");
    hipLaunchKernelGGL(icv::k_knn_sort_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       indptr, n, cols_in, vals_in, cols, vals);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // extern "C"

// ---- tl.leiden (csrc/icv_leiden.hpp) ---------------------------------------------------------------------------------
namespace {
struct LdGeom {
    // two level graphs (A, B: ping-pong above level 0), the per-vertex arrays, the sort buffers of the aggregation
    size_t rp[2], col[2], w[2], loop[2], k, comm[2], K, cnt, sub, Ks, cs, ext, want, wantw, sel, o2c, fa, fb, ra, rb, fl, ll,
        hk, hv, keys[2], vals[2], counters, bytes;
    LdGeom(int64_t n, int64_t nnz) {
        Seg seg;
        const size_t N = (size_t)n + 1, Z = (size_t)nnz + 1;
        for (int i = 0; i < 2; ++i) {
            rp[i] = seg(N * 8), col[i] = seg(Z * 4), w[i] = seg(Z * 8), loop[i] = seg(N * 8), comm[i] = seg(N * 4);
            keys[i] = seg(Z * 8), vals[i] = seg(Z * 8);
        }
        k = seg(N * 8), K = seg(N * 8), cnt = seg(N * 4), sub = seg(N * 4), Ks = seg(N * 8), cs = seg(N * 4);
        ext = seg(N * 8), want = seg(N * 4), wantw = seg(N * 8), sel = seg(N * 4), o2c = seg(N * 4);
        fa = seg(N * 4), fb = seg(N * 4), ra = seg(N * 4), rb = seg(N * 4), fl = seg(N * 4), ll = seg(N * 4);
        hk = seg(2 * Z * 4), hv = seg(2 * Z * 8);  // k_ld_decide_long's tables: 2 slots per stored entry
        counters = seg(64);
        bytes = seg.o;
    }
};
// exclusive prefix sums of m int32 flags (rocprim; its temporary comes from the stream's pool)
int ld_scan(const int32_t* in, int32_t* out, size_t m, hipStream_t st) {
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, out, (int32_t)0, m, rocprim::plus<int32_t>(), st));
    AsyncBuf tmp;
    HIP_TRY(tmp.alloc(tb, st));
    HIP_TRY(rocprim::exclusive_scan(tmp.p, tb, in, out, (int32_t)0, m, rocprim::plus<int32_t>(), st));
    return ICV_OK;
}
struct LdLevel {
    int n;
    int64_t nnz;
    const int64_t* rp;
    const int32_t* col;
    const long long* w;
    const long long* loop;  // nullptr at level 0
    int32_t* comm;
};
}  // namespace

extern "C" {

int icv_leiden_workspace(int64_t n, int64_t nnz, int64_t* bytes) {
    if (!bytes || !graph_sizes_ok(n, nnz)) return fail(ICV_ERR_INVALID, "bad leiden_workspace arguments");
    *bytes = (int64_t)LdGeom(n, nnz).bytes;
    return ICV_OK;
}

int icv_leiden_quantise(const int64_t* indptr, const int32_t* indices, const void* data, int32_t dtype, int64_t n,
                        int64_t nnz, int32_t use_weights, int64_t* q_indptr, int32_t* q_indices, int64_t* q_weights,
                        int64_t* result, void* stream) {
    if (!indptr || !q_indptr || !result || !graph_sizes_ok(n, nnz) ||
        (nnz > 0 && (!indices || !data || !q_indices || !q_weights)) || (dtype != ICV_F32 && dtype != ICV_F64))
        return fail(ICV_ERR_INVALID, "bad leiden_quantise arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AsyncBuf wq, keep, flg;
    HIP_TRY(wq.alloc((size_t)(nnz + 1) * 8, st));
    HIP_TRY(keep.alloc((size_t)n * 8, st));
    HIP_TRY(flg.alloc(32, st));
    HIP_TRY(hipMemsetAsync(flg.p, 0, 32, st));
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(static_cast<char*>(flg.p) + 8);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_ld_quantise<T>, ld_grid(n, 4), dim3(256), 0, st, indptr, indices, static_cast<const T*>(data),
                           n, use_weights, wq.as<long long>(), keep.as<long long>(), flg.as<unsigned>(), sums);
    });
    HIP_TRY(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, flg.p, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned f = (unsigned)(h[0] & 0xFFFFFFFFu);
    ICV_TRY(graph_flags_error("tl.leiden", f));
    const unsigned __int128 total = ((unsigned __int128)h[2] << 32) + h[1];
    if ((f & 64) || total >= ((unsigned __int128)1 << 62))
        return fail(ICV_ERR_INVALID,
                    "tl.leiden: the weights are too large (sum of the integer weights must stay below 2^62)");
    ICV_TRY(icv_row_offsets(keep.as<int64_t>(), n, q_indptr, stream));
    if (nnz > 0)
        hipLaunchKernelGGL(icv::k_ld_compact, ld_grid(n, 4), dim3(256), 0, st, indptr, indices, wq.as<long long>(), n,
                           q_indptr, q_indices, reinterpret_cast<long long*>(q_weights));
    HIP_TRY(hipGetLastError());
    int64_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, q_indptr + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    result[0] = kept;
    result[1] = (int64_t)total;
    return ICV_OK;
}

int icv_leiden_iteration(const int64_t* indptr, const int32_t* indices, const int64_t* weights, int64_t n, int64_t nnz,
                         double gom, uint64_t seed, int32_t iteration, int32_t* labels, void* workspace, int32_t* trace,
                         int32_t* n_levels, int64_t* n_moves, int32_t* bound_reached, float* stage_ms, void* stream) {
    if (!indptr || !labels || !workspace || !trace || !n_levels || !n_moves || !bound_reached || !graph_sizes_ok(n, nnz) ||
        (nnz > 0 && (!indices || !weights)) || !(gom >= 0.0) || !(gom <= 1.7976931348623157e308) || iteration < 0)
        return fail(ICV_ERR_INVALID, "bad leiden_iteration arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LdGeom G(n, nnz);
    char* ws = static_cast<char*>(workspace);
#define LD(T, f) reinterpret_cast<T*>(ws + G.f)
    long long *k = LD(long long, k), *K = LD(long long, K), *Ks = LD(long long, Ks), *ext = LD(long long, ext),
              *wantw = LD(long long, wantw);
    int32_t *cnt = LD(int32_t, cnt), *sub = LD(int32_t, sub), *cs = LD(int32_t, cs), *want = LD(int32_t, want),
            *sel = LD(int32_t, sel), *o2c = LD(int32_t, o2c), *fa = LD(int32_t, fa), *fb = LD(int32_t, fb),
            *ra = LD(int32_t, ra), *rb = LD(int32_t, rb), *fl = LD(int32_t, fl), *ll = LD(int32_t, ll), *hk = LD(int32_t, hk);
    long long* hv = LD(long long, hv);
    unsigned* counters = LD(unsigned, counters);  // [0] wanting [1] selected [2] selected to empty [3] long rows
    unsigned long long* moves = reinterpret_cast<unsigned long long*>(counters + 4);
    StageTimer T(st, stage_ms);  // local moving, refinement, aggregation, rest
    HIP_TRY(T.create());

    LdLevel L{(int)n, nnz, indptr, indices, reinterpret_cast<const long long*>(weights), nullptr, LD(int32_t, comm[0])};
    HIP_TRY(hipMemcpyAsync(L.comm, labels, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(icv::k_ld_iota, ld_grid(n), dim3(256), 0, st, n, o2c);
    HIP_TRY(hipMemsetAsync(counters, 0, 64, st));
    *n_moves = 0;
    *bound_reached = 0;
    *n_levels = 0;
    bool done = false;
    for (int level = 0; level < icv::kLdMaxLevels; ++level) {
        const int ln = L.n;
        const int max_rounds = 64 + (ln < 4096 ? ln : 4096);
        // strengths and the starting partition's sums
        HIP_TRY(T.tic());
        HIP_TRY(hipMemsetAsync(K, 0, (size_t)ln * 8, st));
        HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)ln * 4, st));
        HIP_TRY(hipMemsetAsync(counters + 3, 0, 4, st));
        hipLaunchKernelGGL(icv::k_ld_strength, ld_grid(ln, 4), dim3(256), 0, st, L.rp, L.w, L.loop, ln, k, ll, counters + 3);
        hipLaunchKernelGGL(icv::k_ld_init_comm, ld_grid(ln), dim3(256), 0, st, L.comm, k, ln, K, cnt);
        HIP_TRY(hipGetLastError());
        unsigned h[4], n_long = 0;
        HIP_TRY(hipMemcpyAsync(&n_long, counters + 3, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int r_move = 0, r_ref = 0;
        for (;;) {  // ---- local moving
            if (r_move == max_rounds) {
                *bound_reached = 1;
                break;
            }
            HIP_TRY(hipMemsetAsync(counters, 0, 12, st));
            hipLaunchKernelGGL(icv::k_ld_decide<false>, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, L.w, k, L.comm, K,
                               cnt, nullptr, nullptr, nullptr, gom, want, wantw, counters);
            if (n_long)
                hipLaunchKernelGGL(icv::k_ld_decide_long<false>, dim3(n_long), dim3(256), 0, st, ll, L.rp, L.col, L.w, k, L.comm,
                                   K, cnt, nullptr, nullptr, nullptr, gom, hk, hv, want, wantw, counters);
            hipLaunchKernelGGL(icv::k_ld_select, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, L.comm, want,
                               icv::ld_round_base(seed, iteration, level, 0, r_move), 1, sel, counters);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h, counters, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h[0] == 0) break;
            ++r_move;
            if (h[1] == 0) continue;
            if (h[2]) {
                hipLaunchKernelGGL(icv::k_ld_empty_flags, ld_grid(ln + 1), dim3(256), 0, st, ln, cnt, sel, fa, fb);
                ICV_TRY(ld_scan(fa, ra, (size_t)ln + 1, st));
                ICV_TRY(ld_scan(fb, rb, (size_t)ln + 1, st));
                hipLaunchKernelGGL(icv::k_ld_free_list, ld_grid(ln), dim3(256), 0, st, ln, cnt, ra, fl);
                hipLaunchKernelGGL(icv::k_ld_assign_empty, ld_grid(ln), dim3(256), 0, st, ln, ra, rb, fl, sel);
            }
            hipLaunchKernelGGL(icv::k_ld_apply_move, ld_grid(ln), dim3(256), 0, st, ln, sel, k, L.comm, K, cnt, moves);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(T.toc(0));
        HIP_TRY(T.tic());
        // ---- refinement (K is now the communities' K_C)
        hipLaunchKernelGGL(icv::k_ld_refine_init, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, L.w, k, L.comm, sub, Ks,
                           cs, ext);
        for (;;) {
            if (r_ref == max_rounds) {
                *bound_reached = 1;
                break;
            }
            HIP_TRY(hipMemsetAsync(counters, 0, 12, st));
            hipLaunchKernelGGL(icv::k_ld_decide<true>, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, L.w, k, sub, Ks, cs,
                               L.comm, K, ext, gom, want, wantw, counters);
            if (n_long)
                hipLaunchKernelGGL(icv::k_ld_decide_long<true>, dim3(n_long), dim3(256), 0, st, ll, L.rp, L.col, L.w, k, sub, Ks,
                                   cs, L.comm, K, ext, gom, hk, hv, want, wantw, counters);
            hipLaunchKernelGGL(icv::k_ld_select, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, sub, want,
                               icv::ld_round_base(seed, iteration, level, 1, r_ref), 0, sel, counters);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h, counters, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h[0] == 0) break;
            ++r_ref;
            hipLaunchKernelGGL(icv::k_ld_apply_refine, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, L.w, sel, wantw, k,
                               sub, Ks, cs, ext);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(T.toc(1));
        HIP_TRY(T.tic());
        trace[3 * level] = ln;
        trace[3 * level + 1] = r_move;
        trace[3 * level + 2] = r_ref;
        *n_levels = level + 1;
        // ---- aggregation on the refined partition
        hipLaunchKernelGGL(icv::k_ld_used_flags, ld_grid(ln + 1), dim3(256), 0, st, ln, cs, cnt, fa, fb);
        ICV_TRY(ld_scan(fa, ra, (size_t)ln + 1, st));
        ICV_TRY(ld_scan(fb, rb, (size_t)ln + 1, st));
        int32_t n2 = 0;
        HIP_TRY(hipMemcpyAsync(&n2, ra + ln, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n2 == ln) {
            done = true;
            HIP_TRY(T.toc(2));
            break;
        }
        const int nx = (level & 1) ? 0 : 1;  // level 0 reads the caller's graph; buffers alternate above it
        int64_t* rp2 = LD(int64_t, rp[nx]);
        int32_t* col2 = LD(int32_t, col[nx]);
        long long* loop2 = LD(long long, loop[nx]);
        int32_t* comm2 = LD(int32_t, comm[nx]);
        unsigned long long *keys_in = LD(unsigned long long, keys[0]), *keys_out = LD(unsigned long long, keys[1]);
        long long *vals_in = LD(long long, vals[0]), *vals_out = LD(long long, vals[1]);
        long long* w2 = LD(long long, w[nx]);
        HIP_TRY(hipMemsetAsync(loop2, 0, (size_t)n2 * 8, st));
        hipLaunchKernelGGL(icv::k_ld_agg_vertices, ld_grid(ln), dim3(256), 0, st, ln, sub, L.comm, ra, rb, L.loop, comm2,
                           loop2);
        hipLaunchKernelGGL(icv::k_ld_o2c, ld_grid(n), dim3(256), 0, st, n, sub, ra, o2c);
        int64_t nnz2 = 0;
        if (L.nnz > 0) {
            hipLaunchKernelGGL(icv::k_ld_agg_keys, ld_grid(ln, 4), dim3(256), 0, st, ln, L.rp, L.col, L.w, sub, ra, keys_in,
                               vals_in, loop2);
            HIP_TRY(hipGetLastError());
            size_t tb = 0;
            HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, (size_t)L.nnz, 0, 64, st));
            {
                AsyncBuf tmp;
                HIP_TRY(tmp.alloc(tb, st));
                HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, keys_in, keys_out, vals_in, vals_out, (size_t)L.nnz, 0, 64, st));
            }
            // unique keys -> keys_in, their sums -> w2, count -> counters + 8
            unsigned* n_unique = counters + 8;
            HIP_TRY(rocprim::reduce_by_key(nullptr, tb, keys_out, vals_out, (size_t)L.nnz, keys_in, w2, n_unique,
                                           rocprim::plus<long long>(), rocprim::equal_to<unsigned long long>(), st));
            {
                AsyncBuf tmp;
                HIP_TRY(tmp.alloc(tb, st));
                HIP_TRY(rocprim::reduce_by_key(tmp.p, tb, keys_out, vals_out, (size_t)L.nnz, keys_in, w2, n_unique,
                                               rocprim::plus<long long>(), rocprim::equal_to<unsigned long long>(), st));
            }
            unsigned hu = 0;
            unsigned long long last = 0;
            HIP_TRY(hipMemcpyAsync(&hu, n_unique, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&last, keys_out + (L.nnz - 1), 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            nnz2 = (int64_t)hu - (last == ~0ull ? 1 : 0);  // the entries inside a vertex share the last key
            if (nnz2 > 0) hipLaunchKernelGGL(icv::k_ld_agg_cols, ld_grid(nnz2), dim3(256), 0, st, nnz2, keys_in, col2);
        }
        hipLaunchKernelGGL(icv::k_ld_agg_rowptr, ld_grid(n2 + 1), dim3(256), 0, st, n2, nnz2, keys_in, rp2);
        HIP_TRY(hipGetLastError());
        L = LdLevel{n2, nnz2, rp2, col2, w2, loop2, comm2};
        HIP_TRY(T.toc(2));
    }
    if (!done) *bound_reached = 1;
    HIP_TRY(T.tic());
    hipLaunchKernelGGL(icv::k_ld_gather, ld_grid(n), dim3(256), 0, st, n, L.comm, o2c, labels);
    HIP_TRY(hipGetLastError());
    unsigned long long hm = 0;
    HIP_TRY(hipMemcpyAsync(&hm, moves, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(T.toc(3));
    *n_moves = (int64_t)hm;
    if (stage_ms)
        for (int i = 0; i < 4; ++i) stage_ms[i] = T.ms[i];
#undef LD
    return ICV_OK;
}

int icv_leiden_sums(const int64_t* indptr, const int32_t* indices, const int64_t* weights, int64_t n,
                    const int32_t* labels, int64_t* e, int64_t* K, void* stream) {
    if (!indptr || !labels || !e || !K || n < 1) return fail(ICV_ERR_INVALID, "bad leiden_sums arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(e, 0, (size_t)n * 8, st));
    HIP_TRY(hipMemsetAsync(K, 0, (size_t)n * 8, st));
    hipLaunchKernelGGL(icv::k_ld_sums, ld_grid(n, 4), dim3(256), 0, st, n, indptr, indices,
                       reinterpret_cast<const long long*>(weights), labels, reinterpret_cast<long long*>(e),
                       reinterpret_cast<long long*>(K));
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_leiden_renumber(const int32_t* labels, int64_t n, int32_t* out, int32_t* n_communities, void* stream) {
    if (!labels || !out || !n_communities || n < 1 || n > (int64_t)1 << 30)
        return fail(ICV_ERR_INVALID, "bad leiden_renumber arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AsyncBuf buf;
    const size_t N = ((size_t)n + 63) / 64 * 64;
    HIP_TRY(buf.alloc(N * (4 + 4 + 8 + 8 + 4 + 4 + 4) + 64, st));
    char* p = static_cast<char*>(buf.p);
    unsigned long long *keys = reinterpret_cast<unsigned long long*>(p), *keys2 = keys + N;
    int32_t *size = reinterpret_cast<int32_t*>(keys2 + N), *first = size + N, *ids = first + N, *ids2 = ids + N,
            *rank = ids2 + N;
    unsigned* nc = reinterpret_cast<unsigned*>(rank + N);
    HIP_TRY(hipMemsetAsync(size, 0, N * 4, st));
    HIP_TRY(hipMemsetAsync(first, 0x7f, N * 4, st));
    HIP_TRY(hipMemsetAsync(nc, 0, 4, st));
    hipLaunchKernelGGL(icv::k_ld_sizes, ld_grid(n), dim3(256), 0, st, n, labels, size, first);
    hipLaunchKernelGGL(icv::k_ld_size_keys, ld_grid(n), dim3(256), 0, st, n, size, first, keys, ids, nc);
    HIP_TRY(hipGetLastError());
    size_t tb = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, keys, keys2, ids, ids2, (size_t)n, 0, 64, st));
    {
        AsyncBuf tmp;
        HIP_TRY(tmp.alloc(tb, st));
        HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, keys, keys2, ids, ids2, (size_t)n, 0, 64, st));
    }
    hipLaunchKernelGGL(icv::k_ld_scatter_rank, ld_grid(n), dim3(256), 0, st, n, ids2, rank);
    hipLaunchKernelGGL(icv::k_ld_gather, ld_grid(n), dim3(256), 0, st, n, rank, labels, out);
    HIP_TRY(hipGetLastError());
    unsigned h = 0;
    HIP_TRY(hipMemcpyAsync(&h, nc, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_communities = (int32_t)h;
    return ICV_OK;
}

}  // extern "C"

// ---- tl.umap (csrc/icv_umap.hpp) ---------------------------------------------------------------------------------------
namespace {
struct UmGeom {
    size_t y2, long_list, head, bytes;  // the second position buffer, the long rows, flags / count / largest weight
    UmGeom(int64_t n, int32_t c) {
        Seg seg;
        y2 = seg((size_t)n * c * 4), long_list = seg(((size_t)n + 1) * 4), head = seg(64);
        bytes = seg.o;
    }
};
inline bool um_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }
}  // namespace

extern "C" {

int icv_umap_workspace(int64_t n, int64_t nnz, int32_t n_components, int64_t* bytes) {
    if (!bytes || !graph_sizes_ok(n, nnz) || !components_ok(n_components))
        return fail(ICV_ERR_INVALID, "bad umap_workspace arguments");
    *bytes = (int64_t)UmGeom(n, n_components).bytes;
    return ICV_OK;
}

int icv_umap_epochs(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t nnz,
                    int32_t n_components, double a, double b, double gamma, int32_t negative_sample_rate,
                    double initial_alpha, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, uint64_t seed, float* y,
                    void* workspace, float* stage_ms, void* stream) {
    if (!indptr || !y || !workspace || !graph_sizes_ok(n, nnz) || (nnz > 0 && (!indices || !data)) ||
        !components_ok(n_components) || !um_finite(a) || !(a > 0.0) ||
        !um_finite(b) || !(b > 0.0) || !um_finite(gamma) || !(gamma >= 0.0) || negative_sample_rate < 0 ||
        negative_sample_rate > icv::kUmMaxNegatives || !um_finite(initial_alpha) || !(initial_alpha >= 0.0) ||
        n_epochs < 1 || epoch_begin < 0 || epoch_end < epoch_begin || epoch_end > n_epochs)
        return fail(ICV_ERR_INVALID, "bad umap_epochs arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const UmGeom G(n, n_components);
    char* ws = static_cast<char*>(workspace);
    float* y2 = reinterpret_cast<float*>(ws + G.y2);
    int32_t* long_list = reinterpret_cast<int32_t*>(ws + G.long_list);
    unsigned* head = reinterpret_cast<unsigned*>(ws + G.head);
    StageTimer T(st, stage_ms);  // validation, epochs
    HIP_TRY(T.create());

    GraphCheck chk;
    HIP_TRY(T.tic());
    ICV_TRY(run_graph_check(indptr, indices, data, n, head, long_list, st, &chk));
    HIP_TRY(T.toc(0));
    ICV_TRY(graph_flags_error("tl.umap", chk.flags));
    const unsigned n_long = chk.n_long;
    const float w_max = chk.w_max;

    icv::UmEpoch P;
    P.a = a, P.b = b, P.c_att = (-2.0 * a) * b, P.c_rep = (2.0 * gamma) * b;
    P.w_max = (double)w_max, P.w_min = (double)w_max / (double)n_epochs;
    P.n = n, P.r = negative_sample_rate;
    const unsigned short_blocks = (unsigned)((n + 3) / 4);
    const dim3 grid(short_blocks + n_long);
    float *src = y, *dst = y2;
    HIP_TRY(T.tic());
    for (int32_t t = epoch_begin < 1 ? 1 : epoch_begin; t < epoch_end; ++t) {  // nothing is active in epoch 0
        P.alpha = initial_alpha * (1.0 - (double)t / (double)n_epochs);
        P.t = (double)t, P.tm1 = (double)(t - 1);
        P.base = icv::ld_mix(seed ^ icv::ld_mix((uint64_t)t));
        if (n_components == 2)
            hipLaunchKernelGGL(icv::k_um_epoch<2>, grid, dim3(256), 0, st, indptr, indices, data, src, dst, long_list,
                               short_blocks, P);
        else
            hipLaunchKernelGGL(icv::k_um_epoch<3>, grid, dim3(256), 0, st, indptr, indices, data, src, dst, long_list,
                               short_blocks, P);
        std::swap(src, dst);
    }
    HIP_TRY(hipGetLastError());
    if (src != y) HIP_TRY(hipMemcpyAsync(y, src, (size_t)n * n_components * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(T.toc(1));
    if (stage_ms) stage_ms[0] = T.ms[0], stage_ms[1] = T.ms[1];
    return ICV_OK;
}

}  // extern "C"

// ---- tl.tsne (csrc/icv_tsne.hpp) ---------------------------------------------------------------------------------------
namespace {
struct TsGeom {
    // the second state buffers, two sets of accumulators (row normalisers, repulsion sums, the two halves of Z), the
    // tickets of k_ts_repulse, the long rows, flags / count / longest row
    size_t y2, u2, g2, zr[2], rr[2], hl[2], ticket, long_list, head, bytes, zero_begin, zero_end;
    TsGeom(int64_t n, int32_t c) {
        Seg seg;
        y2 = seg((size_t)n * c * 4), u2 = seg((size_t)n * c * 4), g2 = seg((size_t)n * c * 4);
        zero_begin = seg.o;
        for (int s = 0; s < 2; ++s) zr[s] = seg((size_t)n * 8), rr[s] = seg((size_t)n * c * 8), hl[s] = seg(256);
        ticket = seg(((size_t)n + 255) / 256 * 4);
        zero_end = seg.o;
        long_list = seg(((size_t)n + 1) * 4), head = seg(256);
        bytes = seg.o;
    }
};
}  // namespace

extern "C" {

int icv_tsne_affinities(const float* knn_dist, int64_t n, int32_t k, double perplexity, double* beta, double* cond,
                        void* stream) {
    if (!knn_dist || !beta || !cond || n < 1 || k < 1 || k > 63 || !(perplexity > 0.0) || !(perplexity < (double)k))
        return fail(ICV_ERR_INVALID, "bad tsne_affinities arguments");
    hipLaunchKernelGGL(icv::k_ts_affinity, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       knn_dist, n, k, std::log(perplexity), beta, cond);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_tsne_symmetrize_count(const int32_t* knn_idx, const double* cond, int64_t n, int32_t k, int64_t* row_nnz,
                              void* stream) {
    if (!knn_idx || !cond || !row_nnz || n < 1 || k < 1 || k > 63)
        return fail(ICV_ERR_INVALID, "bad tsne_symmetrize_count arguments");
    return symmetrize_count<true>(knn_idx, cond, n, k, row_nnz, static_cast<hipStream_t>(stream));
}

int icv_tsne_symmetrize_fill(const int32_t* knn_idx, const double* cond, int64_t n, int32_t k, const int64_t* indptr,
                             int64_t nnz, int32_t* indices, float* data, void* stream) {
    if (!knn_idx || !cond || !indptr || !indices || !data || n < 1 || k < 1 || k > 63 || nnz < 0 || nnz > 2 * n * (int64_t)k)
        return fail(ICV_ERR_INVALID, "bad tsne_symmetrize_fill arguments");
    return symmetrize_fill<true>(knn_idx, cond, n, k, indptr, nnz, indices, data, static_cast<hipStream_t>(stream));
}

int icv_tsne_workspace(int64_t n, int64_t nnz, int32_t n_components, int64_t* bytes) {
    if (!bytes || !graph_sizes_ok(n, nnz) || !components_ok(n_components))
        return fail(ICV_ERR_INVALID, "bad tsne_workspace arguments");
    *bytes = (int64_t)TsGeom(n, n_components).bytes;
    return ICV_OK;
}

int icv_tsne_iterations(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t nnz,
                        int32_t n_components, double early_exaggeration, int32_t exaggeration_iters, double learning_rate,
                        int32_t iter_begin, int32_t iter_end, float* y, float* update, float* gains, void* workspace,
                        float* stage_ms, void* stream) {
    if (!indptr || !y || !update || !gains || !workspace || !graph_sizes_ok(n, nnz) ||
        (nnz > 0 && (!indices || !data)) || !components_ok(n_components) ||
        !um_finite(early_exaggeration) || !(early_exaggeration > 0.0) || !um_finite(learning_rate) ||
        !(learning_rate > 0.0) || exaggeration_iters < 0 || iter_begin < 0 || iter_end < iter_begin)
        return fail(ICV_ERR_INVALID, "bad tsne_iterations arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t C = n_components;
    const TsGeom G(n, C);
    char* ws = static_cast<char*>(workspace);
    int32_t* long_list = reinterpret_cast<int32_t*>(ws + G.long_list);
    unsigned* head = reinterpret_cast<unsigned*>(ws + G.head);
    unsigned* ticket = reinterpret_cast<unsigned*>(ws + G.ticket);
    auto u64 = [&](size_t at) { return reinterpret_cast<unsigned long long*>(ws + at); };
    StageTimer T(st, stage_ms);  // validation, iterations
    HIP_TRY(T.create());

    GraphCheck chk;
    HIP_TRY(T.tic());
    ICV_TRY(run_graph_check(indptr, indices, data, n, head, long_list, st, &chk));
    HIP_TRY(T.toc(0));
    ICV_TRY(graph_flags_error("tl.tsne", chk.flags));
    if (chk.w_max > 2.0f)
        return fail(ICV_ERR_INVALID, "tl.tsne: the adjacency matrix has values above 2 (affinities are at most 2)");
    if (chk.longest > icv::kTsMaxRow) return fail(ICV_ERR_UNSUPPORTED, "tl.tsne: a row has more than 2^22 stored entries");
    const unsigned n_long = chk.n_long;

    // the j range is split so that the grid has about 2048 workgroups (8 per CU), in whole tiles
    const int64_t i_blocks = (n + 255) / 256;
    int64_t split = (2048 + i_blocks - 1) / i_blocks;
    const int64_t tiles = (n + icv::kTsTile - 1) / icv::kTsTile;
    split = split < 1 ? 1 : (split > tiles ? tiles : split);
    split = split > 65535 ? 65535 : split;
    const int64_t chunk = (tiles + split - 1) / split * icv::kTsTile;
    const dim3 rgrid((unsigned)i_blocks, (unsigned)((n + chunk - 1) / chunk));
    const unsigned short_blocks = (unsigned)((n + 3) / 4);
    const dim3 sgrid(short_blocks + n_long);
    icv::TsStep P;
    P.eta = learning_rate, P.n = n;
    float *sy = y, *su = update, *sg = gains;
    float *dy = reinterpret_cast<float*>(ws + G.y2), *du = reinterpret_cast<float*>(ws + G.u2),
          *dg = reinterpret_cast<float*>(ws + G.g2);
    HIP_TRY(T.tic());
    HIP_TRY(hipMemsetAsync(ws + G.zero_begin, 0, G.zero_end - G.zero_begin, st));
    int cur = 0;
    for (int32_t t = iter_begin; t < iter_end; ++t, cur ^= 1) {
        const bool early = t < exaggeration_iters;
        P.coef = (early ? early_exaggeration : 1.0) / (2.0 * (double)n);
        P.mom = early ? 0.5 : 0.8;
        unsigned long long *zr = u64(G.zr[cur]), *rr = u64(G.rr[cur]), *hl = u64(G.hl[cur]);
        unsigned long long *zr_n = u64(G.zr[cur ^ 1]), *rr_n = u64(G.rr[cur ^ 1]), *hl_n = u64(G.hl[cur ^ 1]);
        if (C == 2) {
            hipLaunchKernelGGL(icv::k_ts_repulse<2>, rgrid, dim3(256), 0, st, sy, n, chunk, zr, rr, hl, ticket);
            hipLaunchKernelGGL(icv::k_ts_step<2>, sgrid, dim3(256), 0, st, indptr, indices, data, long_list, short_blocks, P,
                               rr, hl, zr_n, rr_n, hl_n, sy, su, sg, dy, du, dg);
        } else {
            hipLaunchKernelGGL(icv::k_ts_repulse<3>, rgrid, dim3(256), 0, st, sy, n, chunk, zr, rr, hl, ticket);
            hipLaunchKernelGGL(icv::k_ts_step<3>, sgrid, dim3(256), 0, st, indptr, indices, data, long_list, short_blocks, P,
                               rr, hl, zr_n, rr_n, hl_n, sy, su, sg, dy, du, dg);
        }
        std::swap(sy, dy), std::swap(su, du), std::swap(sg, dg);
    }
    HIP_TRY(hipGetLastError());
    if (sy != y) {
        const size_t bytes = (size_t)n * C * 4;
        HIP_TRY(hipMemcpyAsync(y, sy, bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(update, su, bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(gains, sg, bytes, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(T.toc(1));
    if (stage_ms) stage_ms[0] = T.ms[0], stage_ms[1] = T.ms[1];
    return ICV_OK;
}

}  // extern "C"

// ---- the chain kernels of the HMM functions (csrc/icv_hmm.hpp): what their entry points share --------------------------------
namespace {

// The argument checks of icv_states_viterbi, icv_posterior_chains, icv_posterior_stats, icv_copy_states_viterbi,
// icv_copy_posterior_chains and icv_copy_posterior_stats, in the order they are reported.
// who: the entry point without icv_; outputs_ok: its own pointers; cap, lds_per_window: its window cap and the LDS bytes a
// window takes (cap_note: what the two depend on, for the message; a cap of 0, where what does not depend on the windows
// fills the LDS alone, refuses every n_cols); params_ok, params_rule: its verdict on the model's scalars and the words
// for it.
int hmm_check(const std::string& who, const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, bool outputs_ok, int cap,
              int lds_per_window, bool params_ok, const char* params_rule, const std::string& cap_note = "") {
    if (!matrix_header_ok(m) || !chr_start || !outputs_ok || n_chr < 1)
        return fail(ICV_ERR_INVALID, "bad " + who + " arguments");
    if (m->n_cols < 1 || m->n_cols > cap)
        return fail(ICV_ERR_INVALID, who + ": n_cols = " + std::to_string(m->n_cols) + " must lie in [1, " +
                                         std::to_string(cap) + "] (" + std::to_string(lds_per_window) +
                                         " bytes of LDS per window" + cap_note + ")");
    if (n_chr > m->n_cols) return fail(ICV_ERR_INVALID, who + ": more chromosomes than windows");
    if (!params_ok) return fail(ICV_ERR_INVALID, who + ": " + params_rule);
    if (!matrix_complete(m) || (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, who + ": incomplete matrix");
    if (m->n_rows > 0x7fffffffLL) return fail(ICV_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 rows in one call");
    return ICV_OK;
}

// the rule of icv_posterior_chains and icv_posterior_stats for (amplitude, h, ps, pw)
bool po_params_ok(double amplitude, double h, double ps, double pw) {
    return std::isfinite(amplitude) && amplitude > 0.0 && std::isfinite(h) && h > 0.0 && std::isnormal(pw) && pw > 0.0 &&
           ps > 0.0 && ps < 1.0 && pw < 0.5;
}
constexpr const char* kPoParamsRule =
    "amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64";

// A chain kernel over the rows of m, one wavefront per row, with lds bytes of dynamic LDS.  pick(t, csr) returns the kernel's
// instantiation for the element type of t and the format (by_matrix); args: what the kernel takes after
// (val, indptr, indices, ld, W, chr_start, C)
template <typename Pick, typename... Args>
int hmm_launch(Pick pick, const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, size_t lds, void* stream, Args... args) {
    if (m->n_rows == 0) return ICV_OK;
    return by_matrix(m, [&](auto t, auto csr) {
        auto kern = pick(t, csr);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)m->n_rows), dim3(64), lds, static_cast<hipStream_t>(stream),
                           (const decltype(t)*)m->values, m->indptr, m->indices, m->ld, m->n_cols, chr_start, n_chr, args...);
        HIP_TRY(hipGetLastError());
        return (int)ICV_OK;
    });
}

}  // namespace

extern "C" {

// ---- tl.cnv_states ---------------------------------------------------------------------------------------
static_assert(icv::kStMaxWindows == ICV_STATES_MAX_WINDOWS, "the header's window cap is the kernel's");
static_assert((size_t)icv::kStMaxWindows * icv::kStLdsPerWindow <= (size_t)icv::kLdsLimit, "one cell fits a CU's LDS");

int icv_states_rowsq(const icv_matrix* m, double* rowsq, int32_t* nonfinite, void* stream) {
    if (!matrix_header_ok(m) || !rowsq || !nonfinite || m->n_cols < 0 || (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, "bad states_rowsq arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(nonfinite, 0, sizeof(int32_t), st));
    if (m->n_rows == 0) return ICV_OK;
    if (!matrix_complete(m) && (m->format == ICV_CSR || m->n_cols > 0))  // (a dense matrix of no columns has no values)
        return fail(ICV_ERR_INVALID, "states_rowsq: incomplete matrix");
    const dim3 grid((unsigned)((m->n_rows + 255) / 256)), block(256);
    by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        if constexpr (decltype(csr)::value)
            hipLaunchKernelGGL(icv::k_states_rowsq_csr<T>, grid, block, 0, st, (const T*)m->values, m->indptr, m->n_rows, rowsq,
                               nonfinite);
        else
            hipLaunchKernelGGL(icv::k_states_rowsq_dense<T>, grid, block, 0, st, (const T*)m->values, m->ld, m->n_rows,
                               m->n_cols, rowsq, nonfinite);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_states_viterbi(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, double amplitude, double h,
                       double stay, double sw, int8_t* states, int32_t* nonneutral, void* stream) {
    const bool params_ok = std::isfinite(amplitude) && amplitude > 0.0 && std::isfinite(h) && h > 0.0 &&
                           std::isfinite(stay) && std::isfinite(sw);
    ICV_TRY(hmm_check("states_viterbi", m, chr_start, n_chr, states && nonneutral, ICV_STATES_MAX_WINDOWS,
                      icv::kStLdsPerWindow, params_ok, "amplitude and h must be finite and > 0, stay and sw finite"));
    return hmm_launch([](auto t, auto csr) { return icv::k_states_viterbi<decltype(t), decltype(csr)::value>; }, m, chr_start,
                      n_chr, icv::st_lds_bytes(m->n_cols), stream, icv::StParams{amplitude, h, stay, sw}, states, nonneutral);
}

int icv_states_fraction(const int32_t* nonneutral, int64_t n_rows, int32_t n_cols, double* fraction, void* stream) {
    if (!nonneutral || !fraction || n_rows < 0 || n_cols < 1) return fail(ICV_ERR_INVALID, "bad states_fraction arguments");
    if (n_rows == 0) return ICV_OK;
    hipLaunchKernelGGL(icv::k_states_fraction, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), nonneutral, n_rows, n_cols, fraction);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_segments -------------------------------------------------------------------------------------
namespace {

// the chromosome-start bit mask of one call (rules 1 of the contract), in a temporary of the stream
int seg_chr_mask(const int32_t* chr_start, int32_t n_chr, int32_t n_cols, AsyncBuf& mask, hipStream_t st) {
    const size_t bytes = icv::seg_mask_words(n_cols) * sizeof(uint32_t);
    HIP_TRY(mask.alloc(bytes, st));
    HIP_TRY(hipMemsetAsync(mask.p, 0, bytes, st));
    hipLaunchKernelGGL(icv::k_seg_chr_mask, dim3((unsigned)((n_chr + 255) / 256)), dim3(256), 0, st, chr_start, n_chr,
                       n_cols, mask.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

bool seg_bad_shape(const void* states, int64_t n_rows, int32_t n_cols, const int32_t* chr_start, int32_t n_chr) {
    return !states || !chr_start || n_rows < 0 || n_cols < 1 || n_chr < 1 || n_chr > n_cols;
}

constexpr int64_t kSegMaxBlocks = 0x7fffffffLL;

// what icv_states_filter and icv_copy_states_filter do after their own pointer checks; who: the entry point without icv_;
// sign: the second plane of icv_copy_states_filter (k_copy_states_filter), null for icv_states_filter (k_states_filter)
int filter_launch(const char* who, const int8_t* states, const double* p_neutral, int64_t n_rows, int32_t n_cols,
                  const int32_t* chr_start, int32_t n_chr, double max_p_normal, int8_t* filtered, int8_t* sign,
                  int32_t* nonneutral, int32_t* removed, int32_t* bad, void* stream) {
    if (n_cols > ICV_FILTER_MAX_WINDOWS)
        return fail(ICV_ERR_UNSUPPORTED, std::string(who) + ": n_cols = " + std::to_string(n_cols) + " is above " +
                                             std::to_string(ICV_FILTER_MAX_WINDOWS) + " (the int64 sum of a run)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n_rows == 0) return ICV_OK;
    const int64_t blocks = (n_rows + icv::kFiRowsPerBlock - 1) / icv::kFiRowsPerBlock;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, std::string(who) + ": too many rows for one call");
    AsyncBuf mask;
    ICV_TRY(seg_chr_mask(chr_start, n_chr, n_cols, mask, st));
    const dim3 grid((unsigned)blocks), block(64 * icv::kFiRowsPerBlock);
    if (sign)
        hipLaunchKernelGGL(icv::k_copy_states_filter, grid, block, 0, st, states, p_neutral, n_rows, n_cols,
                           mask.as<uint32_t>(), max_p_normal, filtered, sign, nonneutral, removed, bad);
    else
        hipLaunchKernelGGL(icv::k_states_filter, grid, block, 0, st, states, p_neutral, n_rows, n_cols,
                           mask.as<uint32_t>(), max_p_normal, filtered, nonneutral, removed, bad);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// k_seg_rows<fill> over all rows with the chromosome mask of the call; who: the entry point without icv_.  levels: the
// count flags what lies outside [lo, hi] instead of what is not -1 / 0 / +1 (the fill validates nothing: one kernel)
int seg_rows_launch(bool fill, const char* who, const int8_t* states, int64_t n_rows, int32_t n_cols, const int32_t* chr_start,
                    int32_t n_chr, hipStream_t st, int64_t* counts, int32_t* bad, const int64_t* offsets, int64_t n_segments,
                    int64_t* seg_row, int32_t* seg_start, int32_t* seg_end, int8_t* seg_state, bool levels = false,
                    int32_t lo = -1, int32_t hi = 1) {
    const int64_t blocks = (n_rows + icv::kSegRowsPerBlock - 1) / icv::kSegRowsPerBlock;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, std::string(who) + ": too many rows for one call");
    AsyncBuf mask;
    ICV_TRY(seg_chr_mask(chr_start, n_chr, n_cols, mask, st));
    const auto kernel = fill ? icv::k_seg_rows<true> : levels ? icv::k_seg_rows<false, true> : icv::k_seg_rows<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * icv::kSegRowsPerBlock), 0, st, states, n_rows, n_cols,
                       mask.as<uint32_t>(), counts, bad, offsets, n_segments, seg_row, seg_start, seg_end, seg_state, lo, hi);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // namespace

int icv_segments_count(const int8_t* states, int64_t n_rows, int32_t n_cols, const int32_t* chr_start, int32_t n_chr,
                       int64_t* counts, int32_t* bad, void* stream) {
    if (seg_bad_shape(states, n_rows, n_cols, chr_start, n_chr) || !counts || !bad)
        return fail(ICV_ERR_INVALID, "bad segments_count arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n_rows == 0) return ICV_OK;
    return seg_rows_launch(false, "segments_count", states, n_rows, n_cols, chr_start, n_chr, st, counts, bad, nullptr, 0,
                           nullptr, nullptr, nullptr, nullptr);
}

int icv_segments_fill(const int8_t* states, int64_t n_rows, int32_t n_cols, const int32_t* chr_start, int32_t n_chr,
                      const int64_t* offsets, int64_t n_segments, int64_t* seg_row, int32_t* seg_start, int32_t* seg_end,
                      int8_t* seg_state, void* stream) {
    if (seg_bad_shape(states, n_rows, n_cols, chr_start, n_chr) || !offsets || n_segments < 0 ||
        (n_segments > 0 && (!seg_row || !seg_start || !seg_end || !seg_state)))
        return fail(ICV_ERR_INVALID, "bad segments_fill arguments");
    if (n_rows == 0 || n_segments == 0) return ICV_OK;
    return seg_rows_launch(true, "segments_fill", states, n_rows, n_cols, chr_start, n_chr, static_cast<hipStream_t>(stream),
                           nullptr, nullptr, offsets, n_segments, seg_row, seg_start, seg_end, seg_state);
}

int icv_state_votes(const int8_t* states, int64_t n_rows, int32_t n_cols, const int64_t* rows, int64_t n_listed,
                    const int64_t* group_ptr, int64_t n_groups, int32_t* loss, int32_t* gain, int32_t* bad, void* stream) {
    if (!states || n_rows < 0 || n_cols < 1 || n_listed < 0 || (n_listed > 0 && !rows) || !group_ptr || n_groups < 0 ||
        (n_groups > 0 && (!loss || !gain)) || !bad)
        return fail(ICV_ERR_INVALID, "bad state_votes arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n_groups == 0) return ICV_OK;
    const size_t table = (size_t)n_groups * (size_t)n_cols * sizeof(int32_t);
    HIP_TRY(hipMemsetAsync(loss, 0, table, st));
    HIP_TRY(hipMemsetAsync(gain, 0, table, st));
    if (n_listed == 0 || n_rows == 0) return ICV_OK;
    const int64_t n_tiles = ((int64_t)n_cols + icv::kVoteTile - 1) / icv::kVoteTile;
    const int64_t blocks = (n_listed + icv::kVoteRows - 1) / icv::kVoteRows * n_tiles;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "state_votes: too many rows x windows for one call");
    hipLaunchKernelGGL(icv::k_state_votes, dim3((unsigned)blocks), dim3(256), 0, st, states, n_rows, n_cols, rows, n_listed,
                       group_ptr, n_groups, (uint32_t)n_tiles, loss, gain, bad);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_state_consensus(const int32_t* loss, const int32_t* gain, const int32_t* need, int64_t n_groups, int32_t n_cols,
                        int8_t* consensus, void* stream) {
    if (n_groups < 0 || n_cols < 1 || (n_groups > 0 && (!loss || !gain || !need || !consensus)))
        return fail(ICV_ERR_INVALID, "bad state_consensus arguments");
    if (n_groups == 0) return ICV_OK;
    const int64_t blocks = (n_groups * (int64_t)n_cols + 255) / 256;
    if (n_groups > kSegMaxBlocks || blocks > kSegMaxBlocks)
        return fail(ICV_ERR_UNSUPPORTED, "state_consensus: too many groups x windows for one call");
    hipLaunchKernelGGL(icv::k_state_consensus, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), loss,
                       gain, need, n_groups, n_cols, consensus);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_segments_support(const int64_t* seg_row, const int32_t* seg_start, const int32_t* seg_end, const int8_t* seg_state,
                         int64_t n_segments, const int32_t* loss, const int32_t* gain, int64_t n_groups, int32_t n_cols,
                         int32_t* cells_min, int64_t* cells_sum, void* stream) {
    if (n_segments < 0 || n_groups < 0 || n_cols < 1 ||
        (n_segments > 0 && (!seg_row || !seg_start || !seg_end || !seg_state || !loss || !gain || !cells_min || !cells_sum)))
        return fail(ICV_ERR_INVALID, "bad segments_support arguments");
    if (n_segments == 0) return ICV_OK;
    const int64_t blocks = (n_segments + 255) / 256;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "segments_support: too many segments for one call");
    hipLaunchKernelGGL(icv::k_seg_support, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), seg_row,
                       seg_start, seg_end, seg_state, n_segments, loss, gain, n_groups, n_cols, cells_min, cells_sum);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_copy_segments --------------------------------------------------------------------------------
static_assert(icv::kLevelMax == ICV_LEVEL_MAX, "the header's level bound is the kernels'");
namespace {

// the rule a level range breaks, or null
const char* level_range_rule(int32_t lo, int32_t hi) {
    return (lo < -ICV_LEVEL_MAX || lo > 0 || hi < 0 || hi > ICV_LEVEL_MAX) ? "-7 <= lo <= 0 <= hi <= 7" : nullptr;
}

int level_range_fail(const char* who, int32_t lo, int32_t hi) {
    return fail(ICV_ERR_INVALID, std::string(who) + ": the level range (" + std::to_string(lo) + ", " + std::to_string(hi) +
                                     ") breaks " + level_range_rule(lo, hi));
}

}  // namespace

int icv_level_segments_count(const int8_t* states, int64_t n_rows, int32_t n_cols, const int32_t* chr_start, int32_t n_chr,
                             int32_t lo, int32_t hi, int64_t* counts, int32_t* bad, void* stream) {
    if (!states || !chr_start || !counts || !bad) return fail(ICV_ERR_INVALID, "level_segments_count: a null pointer");
    if (n_rows < 0 || n_cols < 1) return fail(ICV_ERR_INVALID, "level_segments_count: n_rows >= 0 and n_cols >= 1");
    if (n_chr < 1 || n_chr > n_cols) return fail(ICV_ERR_INVALID, "level_segments_count: 1 <= n_chr <= n_cols");
    if (level_range_rule(lo, hi)) return level_range_fail("level_segments_count", lo, hi);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n_rows == 0) return ICV_OK;
    return seg_rows_launch(false, "level_segments_count", states, n_rows, n_cols, chr_start, n_chr, st, counts, bad, nullptr, 0,
                           nullptr, nullptr, nullptr, nullptr, true, lo, hi);
}

int icv_level_segments_fill(const int8_t* states, int64_t n_rows, int32_t n_cols, const int32_t* chr_start, int32_t n_chr,
                            const int64_t* offsets, int64_t n_segments, int64_t* seg_row, int32_t* seg_start,
                            int32_t* seg_end, int8_t* seg_level, void* stream) {
    if (!states || !chr_start || !offsets || (n_segments > 0 && (!seg_row || !seg_start || !seg_end || !seg_level)))
        return fail(ICV_ERR_INVALID, "level_segments_fill: a null pointer");
    if (n_rows < 0 || n_cols < 1 || n_segments < 0)
        return fail(ICV_ERR_INVALID, "level_segments_fill: n_rows >= 0, n_cols >= 1 and n_segments >= 0");
    if (n_chr < 1 || n_chr > n_cols) return fail(ICV_ERR_INVALID, "level_segments_fill: 1 <= n_chr <= n_cols");
    if (n_rows == 0 || n_segments == 0) return ICV_OK;
    return seg_rows_launch(true, "level_segments_fill", states, n_rows, n_cols, chr_start, n_chr,
                           static_cast<hipStream_t>(stream), nullptr, nullptr, offsets, n_segments, seg_row, seg_start, seg_end,
                           seg_level);
}

int icv_level_votes(const int8_t* states, int64_t n_rows, int32_t n_cols, const int64_t* rows, int64_t n_listed,
                    const int64_t* group_ptr, int64_t n_groups, int32_t lo, int32_t hi, int32_t* counts, int32_t* bad,
                    void* stream) {
    if (!states || (n_listed > 0 && !rows) || !group_ptr || (n_groups > 0 && !counts) || !bad)
        return fail(ICV_ERR_INVALID, "level_votes: a null pointer");
    if (n_rows < 0 || n_cols < 1 || n_listed < 0 || n_groups < 0)
        return fail(ICV_ERR_INVALID, "level_votes: n_rows >= 0, n_cols >= 1, n_listed >= 0 and n_groups >= 0");
    if (level_range_rule(lo, hi)) return level_range_fail("level_votes", lo, hi);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n_groups == 0) return ICV_OK;
    const int planes = hi - lo + 1;
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_groups * (size_t)planes * (size_t)n_cols * sizeof(int32_t), st));
    if (n_listed == 0 || n_rows == 0) return ICV_OK;
    const int64_t n_tiles = ((int64_t)n_cols + icv::kVoteTile - 1) / icv::kVoteTile;
    const int64_t blocks = (n_listed + icv::kVoteRows - 1) / icv::kVoteRows * n_tiles;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "level_votes: too many rows x windows for one call");
    icv::level_votes_launch<1>(planes, dim3((unsigned)blocks), st, states, n_rows, n_cols, rows, n_listed, group_ptr, n_groups,
                          (uint32_t)n_tiles, lo, counts, bad);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_level_consensus(const int32_t* counts, const int32_t* need, int64_t n_groups, int32_t n_cols, int32_t lo, int32_t hi,
                        int32_t* loss, int32_t* gain, int8_t* consensus, void* stream) {
    if (n_groups > 0 && (!counts || !need || !loss || !gain || !consensus))
        return fail(ICV_ERR_INVALID, "level_consensus: a null pointer");
    if (n_groups < 0 || n_cols < 1) return fail(ICV_ERR_INVALID, "level_consensus: n_groups >= 0 and n_cols >= 1");
    if (level_range_rule(lo, hi)) return level_range_fail("level_consensus", lo, hi);
    if (n_groups == 0) return ICV_OK;
    const int64_t blocks = (n_groups * (int64_t)n_cols + 255) / 256;
    if (n_groups > kSegMaxBlocks || blocks > kSegMaxBlocks)
        return fail(ICV_ERR_UNSUPPORTED, "level_consensus: too many groups x windows for one call");
    hipLaunchKernelGGL(icv::k_level_consensus, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), counts,
                       need, n_groups, n_cols, lo, hi, loss, gain, consensus);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_level_segments_support(const int64_t* seg_row, const int32_t* seg_start, const int32_t* seg_end,
                               const int8_t* seg_level, int64_t n_segments, const int32_t* counts, const int32_t* loss,
                               const int32_t* gain, int64_t n_groups, int32_t n_cols, int32_t lo, int32_t hi,
                               int32_t* cells_min, int64_t* cells_sum, int32_t* level_min, int64_t* level_sum, void* stream) {
    if (n_segments > 0 && (!seg_row || !seg_start || !seg_end || !seg_level || !counts || !loss || !gain || !cells_min ||
                           !cells_sum || !level_min || !level_sum))
        return fail(ICV_ERR_INVALID, "level_segments_support: a null pointer");
    if (n_segments < 0 || n_groups < 0 || n_cols < 1)
        return fail(ICV_ERR_INVALID, "level_segments_support: n_segments >= 0, n_groups >= 0 and n_cols >= 1");
    if (level_range_rule(lo, hi)) return level_range_fail("level_segments_support", lo, hi);
    if (n_segments == 0) return ICV_OK;
    const int64_t blocks = (n_segments + 255) / 256;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "level_segments_support: too many segments for one call");
    hipLaunchKernelGGL(icv::k_level_seg_support, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       seg_row, seg_start, seg_end, seg_level, n_segments, counts, loss, gain, n_groups, n_cols, lo, hi,
                       cells_min, cells_sum, level_min, level_sum);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_segments_psum(const double* p_neutral, int64_t n_rows, int32_t n_cols, const int64_t* seg_row,
                      const int32_t* seg_start, const int32_t* seg_end, int64_t n_segments, int64_t* psum, int32_t* bad,
                      void* stream) {
    if (!p_neutral || !bad || (n_segments > 0 && (!seg_row || !seg_start || !seg_end || !psum)))
        return fail(ICV_ERR_INVALID, "segments_psum: a null pointer");
    if (n_rows < 0 || n_cols < 1 || n_segments < 0)
        return fail(ICV_ERR_INVALID, "segments_psum: n_rows >= 0, n_cols >= 1 and n_segments >= 0");
    if (n_cols > ICV_FILTER_MAX_WINDOWS)
        return fail(ICV_ERR_UNSUPPORTED, "segments_psum: n_cols = " + std::to_string(n_cols) + " is above " +
                                             std::to_string(ICV_FILTER_MAX_WINDOWS) + " (the int64 sum of a run)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n_rows == 0 || n_segments == 0) return ICV_OK;
    const int64_t blocks = (n_segments + 255) / 256;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "segments_psum: too many segments for one call");
    hipLaunchKernelGGL(icv::k_seg_psum, dim3((unsigned)blocks), dim3(256), 0, st, p_neutral, n_rows, n_cols, seg_row,
                       seg_start, seg_end, n_segments, psum, bad);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_posteriors and tl.cnv_states_filter -------------------------------------------------------------
static_assert(icv::kPoMaxWindows == ICV_POSTERIOR_MAX_WINDOWS, "the header's window cap is the kernel's");
static_assert((size_t)icv::kPoMaxWindows * icv::kPoLdsPerWindow <= (size_t)icv::kLdsLimit, "one cell fits a CU's LDS");
static_assert(icv::kFiMaxWindows == ICV_FILTER_MAX_WINDOWS, "the header's window cap is the kernel's");

int icv_posterior_chains(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, double amplitude, double h,
                         double ps, double pw, double* neutral, double* loss, double* gain, void* stream) {
    ICV_TRY(hmm_check("posterior_chains", m, chr_start, n_chr, neutral && (loss == nullptr) == (gain == nullptr),
                      ICV_POSTERIOR_MAX_WINDOWS, icv::kPoLdsPerWindow, po_params_ok(amplitude, h, ps, pw), kPoParamsRule));
    return hmm_launch([](auto t, auto csr) { return icv::k_posterior_chains<decltype(t), decltype(csr)::value>; }, m, chr_start,
                      n_chr, icv::po_lds_bytes(m->n_cols), stream, icv::PoParams{amplitude, h, ps, pw}, neutral, loss, gain);
}

int icv_states_filter(const int8_t* states, const double* p_neutral, int64_t n_rows, int32_t n_cols,
                      const int32_t* chr_start, int32_t n_chr, double max_p_normal, int8_t* filtered, int32_t* nonneutral,
                      int32_t* removed, int32_t* bad, void* stream) {
    if (seg_bad_shape(states, n_rows, n_cols, chr_start, n_chr) || !p_neutral || !filtered || !nonneutral || !removed ||
        !bad || !(max_p_normal >= 0.0 && max_p_normal <= 1.0))
        return fail(ICV_ERR_INVALID, "bad states_filter arguments");
    return filter_launch("states_filter", states, p_neutral, n_rows, n_cols, chr_start, n_chr, max_p_normal, filtered, nullptr,
                         nonneutral, removed, bad, stream);
}


// ---- tl.cnv_states_fit: the E-step of the Baum-Welch fit ----------------------------------------------------
int icv_posterior_stats(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, double amplitude, double h, double ps,
                        double pw, double* stats, void* stream) {
    ICV_TRY(hmm_check("posterior_stats", m, chr_start, n_chr, stats != nullptr, ICV_POSTERIOR_MAX_WINDOWS,
                      icv::kPoLdsPerWindow, po_params_ok(amplitude, h, ps, pw), kPoParamsRule));
    return hmm_launch([](auto t, auto csr) { return icv::k_posterior_stats<decltype(t), decltype(csr)::value>; }, m, chr_start,
                      n_chr, icv::po_lds_bytes(m->n_cols), stream, icv::PoParams{amplitude, h, ps, pw}, stats);
}

// ---- tl.cnv_pseudobulk: exact per-group mean profiles -------------------------------------------------------
static_assert((size_t)icv::kPbTile * 12 <= 48 * 1024, "a tile's accumulators take 48 KB of LDS: three workgroups per CU");

int icv_group_profiles(const icv_matrix* m, const int64_t* rows, int64_t n_listed, const int64_t* group_ptr,
                       int64_t n_groups, int32_t shift, int64_t* sum, int32_t* stored, int32_t* flags, void* stream) {
    if (!matrix_header_ok(m) || n_listed < 0 || (n_listed > 0 && !rows) || !group_ptr || n_groups < 0 ||
        (n_groups > 0 && (!sum || !stored)) || !flags || shift < 0 || shift > icv::kPbMaxShift || m->n_cols < 1 ||
        (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, "bad group_profiles arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (n_groups == 0) return ICV_OK;
    const size_t cells = (size_t)n_groups * (size_t)m->n_cols;
    HIP_TRY(hipMemsetAsync(sum, 0, cells * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(stored, 0, cells * sizeof(int32_t), st));
    if (n_listed == 0) return ICV_OK;
    if (!matrix_complete(m) && (m->format == ICV_CSR || m->n_rows > 0))  // (a dense matrix of no rows has no values)
        return fail(ICV_ERR_INVALID, "group_profiles: incomplete matrix");
    // every group of L rows has ceil(L / slab) <= L / slab + 1 slabs, and a group of no rows has none
    const int64_t n_tiles = ((int64_t)m->n_cols + icv::kPbTile - 1) / icv::kPbTile;
    const int64_t max_slabs = n_listed / icv::kPbSlab + std::min(n_groups, n_listed);
    if (max_slabs > kSegMaxBlocks / n_tiles)
        return fail(ICV_ERR_UNSUPPORTED, "group_profiles: too many rows x windows for one call");
    AsyncBuf slabs, slab_off;
    HIP_TRY(slabs.alloc((size_t)n_groups * sizeof(int64_t), st));
    HIP_TRY(slab_off.alloc((size_t)(n_groups + 1) * sizeof(int64_t), st));
    hipLaunchKernelGGL(icv::k_pb_slab_counts, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, group_ptr, n_groups,
                       n_listed, slabs.as<int64_t>());
    HIP_TRY(hipGetLastError());
    ICV_TRY(icv_row_offsets(slabs.as<int64_t>(), n_groups, slab_off.as<int64_t>(), stream));
    const dim3 grid((unsigned)(max_slabs * n_tiles)), block(icv::kPbThreads);
    by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        hipLaunchKernelGGL((icv::k_group_profiles<T, decltype(csr)::value>), grid, block, 0, st, (const T*)m->values, m->indptr,
                           m->indices, m->ld, m->n_rows, m->n_cols, rows, n_listed, group_ptr, n_groups, slab_off.as<int64_t>(),
                           (uint32_t)n_tiles, (int)shift, reinterpret_cast<unsigned long long*>(sum), stored, flags);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_group_profiles_finish(const int64_t* sum, const int32_t* stored, const int64_t* group_ptr, int64_t n_groups,
                              int32_t n_cols, int32_t shift, double* mean, double* fraction, void* stream) {
    if (n_groups < 0 || n_cols < 1 || shift < 0 || shift > icv::kPbMaxShift || !group_ptr ||
        (n_groups > 0 && (!sum || !stored || !mean || !fraction)))
        return fail(ICV_ERR_INVALID, "bad group_profiles_finish arguments");
    if (n_groups == 0) return ICV_OK;
    if (n_groups > kSegMaxBlocks || (n_groups * (int64_t)n_cols + 255) / 256 > kSegMaxBlocks)
        return fail(ICV_ERR_UNSUPPORTED, "group_profiles_finish: too many groups x windows for one call");
    hipLaunchKernelGGL(icv::k_group_profiles_finish, dim3((unsigned)((n_groups * (int64_t)n_cols + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), sum, stored, group_ptr, n_groups, n_cols, (int)shift, mean, fraction);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_correlation / tl.cnv_signal: the rows of X_cnv against centred profiles -------------------------
int icv_profile_corr(const icv_matrix* m, const double* profiles_t, const double* s2, int64_t n_profiles, double* a, double* b,
                     double* signal, double* r, int32_t* flags, void* stream) {
    if (!matrix_header_ok(m) || n_profiles < 0 || (n_profiles > 0 && (!profiles_t || !s2 || !r)) || !a || !b || !signal ||
        !flags || m->n_cols < 1 || (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, "bad profile_corr arguments");
    if (m->n_rows > 0 && !matrix_complete(m)) return fail(ICV_ERR_INVALID, "profile_corr: incomplete matrix");
    const int gp = icv::pc_group_lanes(n_profiles);
    const int64_t blocks = (m->n_rows + icv::kPcThreads / gp - 1) / (icv::kPcThreads / gp);
    const int64_t tiles = std::max<int64_t>(1, (n_profiles + icv::kPcTileG - 1) / icv::kPcTileG);
    if (blocks > kSegMaxBlocks || tiles > 65535)
        return fail(ICV_ERR_UNSUPPORTED, "profile_corr: too many rows or profiles for one call");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (m->n_rows == 0) return ICV_OK;
    const dim3 grid((unsigned)blocks, (unsigned)tiles), block(icv::kPcThreads);
    by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        auto launch = [&](auto lanes) {
            hipLaunchKernelGGL((icv::k_profile_corr<T, decltype(csr)::value, decltype(lanes)::value>), grid, block, 0, st,
                               (const T*)m->values, m->indptr, m->indices, m->ld, m->n_rows, m->n_cols, profiles_t, s2,
                               n_profiles, a, b, signal, r, flags);
        };
        switch (gp) {
            case 1: launch(std::integral_constant<int, 1>{}); break;
            case 8: launch(std::integral_constant<int, 8>{}); break;
            case 16: launch(std::integral_constant<int, 16>{}); break;
            case 32: launch(std::integral_constant<int, 32>{}); break;
            default: launch(std::integral_constant<int, 64>{}); break;
        }
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_profile_corr_best(const double* r, int64_t n_rows, int64_t n_profiles, double* best_r, int32_t* best_g, void* stream) {
    if (n_rows < 0 || n_profiles < 0 || n_profiles > 0x7fffffffLL || (n_rows > 0 && (!best_r || !best_g)) ||
        (n_rows > 0 && n_profiles > 0 && !r))
        return fail(ICV_ERR_INVALID, "bad profile_corr_best arguments");
    if (n_rows == 0) return ICV_OK;
    if ((n_rows + 255) / 256 > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "profile_corr_best: too many rows for one call");
    hipLaunchKernelGGL(icv::k_profile_corr_best, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), r, n_rows, n_profiles, best_r, best_g);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_silhouette: exact silhouette widths from int64 sums of rounded distances ------------------------
static_assert(icv::kSilTileI == ICV_SILHOUETTE_TILE_I && icv::kSilTileJ == ICV_SILHOUETTE_TILE_J &&
                  icv::kSilTileC == ICV_SILHOUETTE_TILE_C && icv::kSilMaxC == ICV_SILHOUETTE_MAX_COMPONENTS &&
                  icv::kSilMaxShift == ICV_SILHOUETTE_MAX_SHIFT,
              "the header's silhouette constants are the kernel's");

int icv_silhouette_sums(const void* x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const int64_t* rows,
                        int64_t n_listed, int64_t i0, int64_t i1, const int64_t* tiles, int64_t n_tiles,
                        const int32_t* chunk_ptr, int32_t n_chunks, int64_t n_groups, int32_t shift, int32_t dist_exp,
                        int64_t* sums, int32_t* flags, void* stream) {
    if ((dtype != ICV_F32 && dtype != ICV_F64) || n_rows < 0 || n_comp < 1 || n_comp > icv::kSilMaxC || ld < n_comp ||
        n_listed < 0 || i0 < 0 || i1 < i0 || i1 > n_listed || i0 % icv::kSilTileI != 0 || n_tiles < 0 ||
        n_tiles > 0x7fffffffLL || n_chunks < 0 || n_groups < 1 || shift < 0 || shift > icv::kSilMaxShift || !flags ||
        (i1 > i0 && (!x || !rows || !sums)) || (n_tiles > 0 && !tiles) || (n_chunks > 0 && !chunk_ptr))
        return fail(ICV_ERR_INVALID, "bad silhouette_sums arguments");
    if (i1 == i0) return ICV_OK;
    if (i1 - i0 > 0x7fffffffffffffffLL / 8 / n_groups) return fail(ICV_ERR_INVALID, "silhouette_sums: the table of sums overflows");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(sums, 0, (size_t)(i1 - i0) * (size_t)n_groups * sizeof(int64_t), st));
    if (n_tiles == 0 || n_chunks == 0) return ICV_OK;
    const int64_t blocks = (i1 - i0 + icv::kSilTileI - 1) / icv::kSilTileI;
    if (blocks > kSegMaxBlocks || n_chunks > 65535)
        return fail(ICV_ERR_UNSUPPORTED, "silhouette_sums: too many positions or chunks for one call");
    const dim3 grid((unsigned)blocks, (unsigned)n_chunks), block(icv::kSilThreads);
    const double scale = std::ldexp(1.0, shift);
    const bool magic = (int64_t)shift + dist_exp <= icv::kSilMagicBits;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto m) {
            hipLaunchKernelGGL((icv::k_sil_sums<T, decltype(m)::value>), grid, block, 0, st, (const T*)x, ld, n_rows,
                               (int)n_comp, rows, n_listed, i0, i1, tiles, n_tiles, chunk_ptr, n_groups, scale,
                               (unsigned long long*)sums, flags);
        };
        if (magic) launch(std::true_type{});
        else launch(std::false_type{});
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_silhouette_finish(const int64_t* sums, int64_t i0, int64_t i1, const int64_t* group_ptr, int64_t n_groups,
                          int32_t shift, double* s, double* a, double* b, int32_t* nearest, void* stream) {
    if (i0 < 0 || i1 < i0 || n_groups < 1 || n_groups > 0x7fffffffLL || shift < 0 || shift > icv::kSilMaxShift ||
        (i1 > i0 && (!sums || !group_ptr || !s || !a || !b || !nearest)))
        return fail(ICV_ERR_INVALID, "bad silhouette_finish arguments");
    if (i1 == i0) return ICV_OK;
    const int64_t blocks = (i1 - i0 + 255) / 256;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "silhouette_finish: too many positions for one call");
    hipLaunchKernelGGL(icv::k_sil_finish, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (const long long*)sums, i0, i1, group_ptr, n_groups, std::ldexp(1.0, shift), s, a, b, nearest);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_kmeans: deterministic exact k-means from integer sums ----------------------------------------
static_assert(icv::kKmTileCells == ICV_KMEANS_TILE_CELLS && icv::kKmTileCentres == ICV_KMEANS_TILE_CENTRES &&
                  icv::kKmTileC == ICV_KMEANS_TILE_C && icv::kKmMaxC == ICV_KMEANS_MAX_COMPONENTS &&
                  icv::kKmMaxK == ICV_KMEANS_MAX_CLUSTERS && icv::kKmMaxShift == ICV_KMEANS_MAX_SHIFT &&
                  icv::kKmSeedRows == ICV_KMEANS_SEED_ROWS && icv::kKmUpdRows == ICV_KMEANS_UPDATE_ROWS &&
                  icv::kKmUpdTileC == ICV_KMEANS_UPDATE_TILE_C,
              "the header's k-means constants are the kernel's");

namespace {
// what every k-means entry checks of the representation
bool kmeans_matrix_ok(const void* x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld) {
    return x && (dtype == ICV_F32 || dtype == ICV_F64) && n_rows >= 1 &&
           n_rows <= kSegMaxBlocks * (int64_t)icv::kKmSeedRows && n_comp >= 1 && n_comp <= icv::kKmMaxC && ld >= n_comp;
}
bool kmeans_shift_ok(int32_t shift) { return shift >= 0 && shift <= icv::kKmMaxShift; }
}  // namespace

int icv_kmeans_seed_dist(const void* x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const double* centre,
                         int32_t first, int32_t shift_f, double* mind, int64_t* w, int64_t* partials, int32_t* flags,
                         void* stream) {
    if (!kmeans_matrix_ok(x, dtype, n_rows, n_comp, ld) || !kmeans_shift_ok(shift_f) || !centre || !mind || !w ||
        !partials || !flags)
        return fail(ICV_ERR_INVALID, "bad kmeans_seed_dist arguments");
    const int64_t blocks = (n_rows + icv::kKmSeedRows - 1) / icv::kKmSeedRows;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_km_seed_dist<T>, dim3((unsigned)blocks), dim3(icv::kKmThreads), 0,
                           static_cast<hipStream_t>(stream), (const T*)x, ld, n_rows, (int)n_comp, centre, (int)(first != 0),
                           std::ldexp(1.0, shift_f), mind, (long long*)w, (unsigned long long*)partials, flags);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_kmeans_seed_pick(const void* x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const int64_t* w,
                         const int64_t* partials, int32_t t, int32_t n_clusters, uint64_t z, double* centres,
                         int64_t* picks, int32_t* flags, void* stream) {
    if (!kmeans_matrix_ok(x, dtype, n_rows, n_comp, ld) || n_clusters < 1 || n_clusters > icv::kKmMaxK || t < 0 ||
        t >= n_clusters || (t > 0 && (!w || !partials)) || !centres || !picks || !flags)
        return fail(ICV_ERR_INVALID, "bad kmeans_seed_pick arguments");
    const int64_t blocks = (n_rows + icv::kKmSeedRows - 1) / icv::kKmSeedRows;
    by_dtype(dtype, [&](auto tt) {
        using T = decltype(tt);
        hipLaunchKernelGGL(icv::k_km_seed_pick<T>, dim3(1), dim3(icv::kKmThreads), 0, static_cast<hipStream_t>(stream),
                           (const T*)x, ld, n_rows, (int)n_comp, (const long long*)w, (const unsigned long long*)partials,
                           blocks, (int)t, (unsigned long long)z, centres, picks, flags);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_kmeans_assign(const void* x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const double* centres,
                      int32_t n_clusters, int32_t shift_f, int32_t* labels, double* sqdist, int64_t* stats, int32_t* flags,
                      void* stream) {
    if (!kmeans_matrix_ok(x, dtype, n_rows, n_comp, ld) || n_clusters < 1 || n_clusters > icv::kKmMaxK ||
        !kmeans_shift_ok(shift_f) || !centres || !labels || !sqdist || !stats || !flags)
        return fail(ICV_ERR_INVALID, "bad kmeans_assign arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), st));
    const int64_t blocks = (n_rows + icv::kKmTileCells - 1) / icv::kKmTileCells;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_km_assign<T>, dim3((unsigned)blocks), dim3(icv::kKmThreads), 0, st, (const T*)x, ld, n_rows,
                           (int)n_comp, centres, (int)n_clusters, std::ldexp(1.0, shift_f), labels, sqdist,
                           (unsigned long long*)stats, flags);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_kmeans_update(const void* x, int32_t dtype, int64_t n_rows, int32_t n_comp, int64_t ld, const int32_t* labels,
                      int32_t n_clusters, int32_t shift_e, int64_t* sums, void* stream) {
    if (!kmeans_matrix_ok(x, dtype, n_rows, n_comp, ld) || n_clusters < 1 || n_clusters > icv::kKmMaxK ||
        !kmeans_shift_ok(shift_e) || !labels || !sums)
        return fail(ICV_ERR_INVALID, "bad kmeans_update arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(sums, 0, (size_t)n_clusters * (size_t)(n_comp + 1) * sizeof(int64_t), st));
    const int64_t slabs = (n_rows + icv::kKmUpdRows - 1) / icv::kKmUpdRows;
    const dim3 grid((unsigned)slabs, (unsigned)((n_comp + icv::kKmUpdTileC - 1) / icv::kKmUpdTileC));
    unsigned long long* q = (unsigned long long*)sums;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(icv::k_km_update<T>, grid, dim3(icv::kKmThreads), 0, st, (const T*)x, ld, n_rows, (int)n_comp,
                           labels, (int)n_clusters, std::ldexp(1.0, shift_e), q, q + (size_t)n_clusters * (size_t)n_comp);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_kmeans_centres(const int64_t* sums, int32_t n_clusters, int32_t n_comp, int32_t shift_e, double* centres,
                       void* stream) {
    if (n_clusters < 1 || n_clusters > icv::kKmMaxK || n_comp < 1 || n_comp > icv::kKmMaxC || !kmeans_shift_ok(shift_e) ||
        !sums || !centres)
        return fail(ICV_ERR_INVALID, "bad kmeans_centres arguments");
    const int cells = n_clusters * n_comp;
    hipLaunchKernelGGL(icv::k_km_centres, dim3((unsigned)((cells + icv::kKmThreads - 1) / icv::kKmThreads)),
                       dim3(icv::kKmThreads), 0, static_cast<hipStream_t>(stream), (const long long*)sums,
                       (const long long*)sums + cells, (int)n_clusters, (int)n_comp, std::ldexp(1.0, shift_e), centres);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_changepoints: exact penalised segmentation of every chromosome of every row -------------------
static_assert(icv::kCpMaxChrWindows == ICV_CHANGEPOINT_MAX_CHR_WINDOWS, "the header's chromosome cap is the kernel's");
static_assert((size_t)(icv::kCpMaxChrWindows + 1) * icv::kCpLdsPerWindow <= (size_t)icv::kLdsLimit,
              "one chromosome fits a CU's LDS");

}  // extern "C"

namespace {

// What icv_changepoint_levels and icv_changepoint_diffsq check and do alike.  who: the entry point without icv_; ok: its
// verdict on its own arguments.  The n_chr + 1 starts are copied to the host (the one synchronisation of the stream) and must
// be ascending from 0 to n_cols with no chromosome above the cap; *longest receives the longest chromosome, which sizes the
// launch's LDS.  ICV_OK with *longest = 0: no rows, nothing to launch.
int cp_check(const std::string& who, const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, bool ok, hipStream_t st,
             int32_t* longest) {
    *longest = 0;
    if (!matrix_header_ok(m) || !chr_start || !ok || n_chr < 1 || m->n_cols < 1 || (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, "bad " + who + " arguments");
    if (n_chr > m->n_cols) return fail(ICV_ERR_INVALID, who + ": more chromosomes than windows");
    if (m->n_rows == 0) return ICV_OK;
    if (!matrix_complete(m)) return fail(ICV_ERR_INVALID, who + ": incomplete matrix");
    if (m->n_rows > kSegMaxBlocks / n_chr)
        return fail(ICV_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 rows x chromosomes in one call");
    std::vector<int32_t> cs((size_t)n_chr + 1);
    HIP_TRY(hipMemcpyAsync(cs.data(), chr_start, cs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (cs.front() != 0 || cs.back() != m->n_cols)
        return fail(ICV_ERR_INVALID, who + ": chr_start must run from 0 to n_cols");
    for (int32_t c = 0; c < n_chr; ++c) {
        if (cs[c + 1] < cs[c]) return fail(ICV_ERR_INVALID, who + ": chr_start must be ascending");
        const int32_t len = cs[c + 1] - cs[c];
        if (len > ICV_CHANGEPOINT_MAX_CHR_WINDOWS)
            return fail(ICV_ERR_INVALID, who + ": a chromosome of " + std::to_string(len) + " windows is above " +
                                             std::to_string(ICV_CHANGEPOINT_MAX_CHR_WINDOWS) + " (" +
                                             std::to_string(icv::kCpLdsPerWindow) + " bytes of LDS per window)");
        *longest = std::max(*longest, len);
    }
    return ICV_OK;
}

// one wavefront per (row, chromosome) with lds bytes of dynamic LDS; pick and args as for hmm_launch
template <typename Pick, typename... Args>
int cp_launch(Pick pick, const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, size_t lds, hipStream_t st, Args... args) {
    return by_matrix(m, [&](auto t, auto csr) {
        auto kern = pick(t, csr);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)(m->n_rows * n_chr)), dim3(64), lds, st, (const decltype(t)*)m->values,
                           m->indptr, m->indices, m->ld, m->n_cols, chr_start, n_chr, args...);
        HIP_TRY(hipGetLastError());
        return (int)ICV_OK;
    });
}

}  // namespace

extern "C" {

int icv_changepoint_levels(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, double beta, int32_t min_windows,
                           double* levels, uint8_t* starts, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t longest = 0;
    ICV_TRY(cp_check("changepoint_levels", m, chr_start, n_chr,
                     levels && starts && std::isfinite(beta) && beta >= 0.0 && min_windows >= 1, st, &longest));
    if (longest == 0) return ICV_OK;
    // (a min_windows above the longest chromosome acts as longest + 1: every chromosome is one segment)
    return cp_launch([](auto t, auto csr) { return icv::k_changepoint_levels<decltype(t), decltype(csr)::value>; }, m,
                     chr_start, n_chr, icv::cp_lds_bytes(longest), st, longest, beta, std::min(min_windows, longest + 1), levels, starts);
}

int icv_changepoint_diffsq(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, double* d, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t longest = 0;
    ICV_TRY(cp_check("changepoint_diffsq", m, chr_start, n_chr, d != nullptr, st, &longest));
    if (longest == 0) return ICV_OK;
    AsyncBuf e;
    HIP_TRY(e.alloc((size_t)m->n_rows * (size_t)n_chr * sizeof(double), st));
    ICV_TRY(cp_launch([](auto t, auto csr) { return icv::k_changepoint_diffsq<decltype(t), decltype(csr)::value>; }, m,
                      chr_start, n_chr, (size_t)longest * 16, st, longest, e.as<double>()));
    hipLaunchKernelGGL(icv::k_changepoint_rowsum, dim3((unsigned)((m->n_rows + 255) / 256)), dim3(256), 0, st, e.as<double>(),
                       m->n_rows, n_chr, d);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_rank_groups: exact doubled mid-rank sums of every group in every window -------------------------
static_assert((size_t)icv::kRkTile * 4 <= 32 * 1024, "the counters of a window tile take 32 KB of LDS");
static_assert((size_t)icv::kRkLdsGroups * 12 + 16 <= 32 * 1024, "the sums of a workgroup take 24 KB of LDS");
static_assert(icv::kRkMaxCells == ICV_RANK_MAX_CELLS, "the header's population cap is the kernel's");
static_assert(icv::kRkChunk % icv::kRkSumThreads == 0, "every thread of the rank sums takes the same share of a chunk");

int icv_rank_count(const icv_matrix* m, const int32_t* code, int32_t* stored, int32_t* flags, void* stream) {
    if (!matrix_header_ok(m) || !stored || !flags || m->n_cols < 1 || (m->n_rows > 0 && !code) ||
        (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, "bad rank_count arguments");
    if (m->n_rows > 0 && !matrix_complete(m)) return fail(ICV_ERR_INVALID, "rank_count: incomplete matrix");
    const int64_t n_tiles = ((int64_t)m->n_cols + icv::kRkTile - 1) / icv::kRkTile;
    const int64_t slabs = (m->n_rows + icv::kRkSlab - 1) / icv::kRkSlab;
    if (slabs > kSegMaxBlocks / n_tiles) return fail(ICV_ERR_UNSUPPORTED, "rank_count: too many rows x windows for one call");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(stored, 0, (size_t)m->n_cols * sizeof(int32_t), st));
    if (m->n_rows == 0) return ICV_OK;
    const dim3 grid((unsigned)(slabs * n_tiles)), block(icv::kRkThreads);
    by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        hipLaunchKernelGGL((icv::k_rank_count<T, decltype(csr)::value>), grid, block, 0, st, (const T*)m->values, m->indptr,
                           m->indices, m->ld, m->n_rows, m->n_cols, code, (uint32_t)n_tiles, stored, flags);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_rank_scatter(const icv_matrix* m, const int32_t* code, int32_t w0, int32_t n_win, const int32_t* seg_off,
                     int32_t* cursor, uint64_t* keys, int32_t* payload, void* stream) {
    if (!matrix_header_ok(m) || m->n_cols < 1 || (m->n_rows > 0 && !code) || w0 < 0 || n_win < 1 || w0 > m->n_cols - n_win ||
        !seg_off || !cursor || !keys || !payload || (m->format == ICV_DENSE && m->ld < m->n_cols))
        return fail(ICV_ERR_INVALID, "bad rank_scatter arguments");
    if (m->n_rows > 0 && !matrix_complete(m)) return fail(ICV_ERR_INVALID, "rank_scatter: incomplete matrix");
    const int64_t n_tiles = ((int64_t)n_win + icv::kRkTile - 1) / icv::kRkTile;
    const int64_t slabs = (m->n_rows + icv::kRkSlab - 1) / icv::kRkSlab;
    if (slabs > kSegMaxBlocks / n_tiles) return fail(ICV_ERR_UNSUPPORTED, "rank_scatter: too many rows x windows for one call");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)n_win * sizeof(int32_t), st));
    if (m->n_rows == 0) return ICV_OK;
    by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        hipLaunchKernelGGL((icv::k_rank_scatter<T, decltype(csr)::value>), dim3((unsigned)(slabs * n_tiles)),
                           dim3(icv::kRkThreads), 0, st, (const T*)m->values, m->indptr, m->indices, m->ld, m->n_rows, code, w0,
                           n_win, (uint32_t)n_tiles, seg_off, cursor, reinterpret_cast<unsigned long long*>(keys), payload);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_rank_sort(const uint64_t* keys, const int32_t* payload, int64_t n_entries, const int32_t* seg_off, int32_t n_win,
                  uint64_t* keys_sorted, int32_t* payload_sorted, void* stream) {
    if (n_entries < 0 || n_entries > 0x7fffffffLL || n_win < 1 || !seg_off ||
        (n_entries > 0 && (!keys || !payload || !keys_sorted || !payload_sorted)))
        return fail(ICV_ERR_INVALID, "bad rank_sort arguments");
    if (n_entries == 0) return ICV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned long long* in = reinterpret_cast<const unsigned long long*>(keys);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(keys_sorted);
    size_t tb = 0;
    HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, tb, in, out, payload, payload_sorted, (unsigned)n_entries,
                                                (unsigned)n_win, seg_off, seg_off + 1, 0, 64, st));
    AsyncBuf tmp;
    HIP_TRY(tmp.alloc(tb, st));
    HIP_TRY(rocprim::segmented_radix_sort_pairs(tmp.p, tb, in, out, payload, payload_sorted, (unsigned)n_entries,
                                                (unsigned)n_win, seg_off, seg_off + 1, 0, 64, st));
    return ICV_OK;
}

int icv_rank_sums(const uint64_t* keys, const int32_t* payload, const int32_t* seg_off, int32_t w0, int32_t n_win,
                  int32_t longest, int32_t n_cols, int64_t n_pop, int32_t n_codes, int64_t* r2, int32_t* cnt, int64_t* tie,
                  int32_t* neg, void* stream) {
    if (!seg_off || w0 < 0 || n_win < 1 || n_cols < 1 || w0 > n_cols - n_win || longest < 0 || n_pop < 0 ||
        n_pop >= ICV_RANK_MAX_CELLS || longest > n_pop || n_codes < 1 || !r2 || !cnt || !tie || !neg ||
        (longest > 0 && (!keys || !payload)))
        return fail(ICV_ERR_INVALID, "bad rank_sums arguments");
    if (longest == 0) return ICV_OK;
    const dim3 grid((unsigned)n_win, (unsigned)((longest + icv::kRkChunk - 1) / icv::kRkChunk)), block(icv::kRkSumThreads);
    auto launch = [&](auto lds) {
        hipLaunchKernelGGL((icv::k_rank_sums<decltype(lds)::value>), grid, block, 0, static_cast<hipStream_t>(stream),
                           reinterpret_cast<const unsigned long long*>(keys), payload, seg_off, w0, n_cols, n_pop, n_codes,
                           reinterpret_cast<unsigned long long*>(r2), cnt, reinterpret_cast<unsigned long long*>(tie), neg);
    };
    if (n_codes <= icv::kRkLdsGroups) launch(std::true_type{}); else launch(std::false_type{});
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_rank_finish(const int32_t* stored, const int32_t* neg, const int32_t* cnt, const int64_t* n_cells, int64_t n_groups,
                    int32_t n_cols, int64_t n_pop, int64_t* r2, int64_t* tie, void* stream) {
    if (n_groups < 0 || n_cols < 1 || n_pop < 0 || n_pop >= ICV_RANK_MAX_CELLS ||
        (n_groups > 0 && (!stored || !neg || !cnt || !n_cells || !r2 || !tie)))
        return fail(ICV_ERR_INVALID, "bad rank_finish arguments");
    if (n_groups == 0) return ICV_OK;
    const int64_t blocks = (n_groups * (int64_t)n_cols + 255) / 256;
    if (n_groups > kSegMaxBlocks || blocks > kSegMaxBlocks)
        return fail(ICV_ERR_UNSUPPORTED, "rank_finish: too many groups x windows for one call");
    hipLaunchKernelGGL(icv::k_rank_finish, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), stored, neg,
                       cnt, n_cells, n_groups, n_cols, n_pop, r2, tie);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

// ---- tl.cnv_pool_neighbors: exact means over every cell's graph neighbourhood -------------------------------
static_assert((size_t)icv::kPoolTile * 8 <= 16 * 1024, "a tile's sums take 16 KB of LDS: ten workgroups per CU");
static_assert(icv::kPoolTile % 2 == 0, "a tile starts at an even window: the 16-byte stores pair windows from there");

int icv_neighbor_pool_sizes(const int64_t* g_indptr, const int32_t* g_indices, int64_t n, int32_t* n_cells, int32_t* flags,
                            void* stream) {
    if (!g_indptr || !g_indices || n < 1 || !n_cells || !flags)
        return fail(ICV_ERR_INVALID, "bad neighbor_pool_sizes arguments");
    constexpr int64_t rows_per_block = icv::kPoolThreads / 64;
    const int64_t blocks = (n + rows_per_block - 1) / rows_per_block;
    if (blocks > kSegMaxBlocks) return fail(ICV_ERR_UNSUPPORTED, "neighbor_pool_sizes: too many cells for one call");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(icv::k_pool_sizes, dim3((unsigned)blocks), dim3(icv::kPoolThreads), 0, st, g_indptr, g_indices, n,
                       n_cells, flags);
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

int icv_neighbor_pool(const icv_matrix* m, const int64_t* g_indptr, const int32_t* g_indices, int64_t n, int32_t shift,
                      const int32_t* n_cells, double* out, int64_t ldo, int32_t* flags, void* stream) {
    if (!matrix_header_ok(m) || !g_indptr || !g_indices || n < 1 || m->n_rows != n || m->n_cols < 1 || shift < 0 ||
        shift > icv::kPbMaxShift || !n_cells || !out || ldo < m->n_cols || !flags ||
        (m->format == ICV_DENSE && m->ld < m->n_cols) || !matrix_complete(m))
        return fail(ICV_ERR_INVALID, "bad neighbor_pool arguments");
    const int64_t n_tiles = ((int64_t)m->n_cols + icv::kPoolTile - 1) / icv::kPoolTile;
    if (n > kSegMaxBlocks / n_tiles) return fail(ICV_ERR_UNSUPPORTED, "neighbor_pool: too many cells x windows for one call");
    const dim3 grid((unsigned)(n * n_tiles)), block(icv::kPoolThreads);
    by_matrix(m, [&](auto t, auto csr) {
        using T = decltype(t);
        hipLaunchKernelGGL((icv::k_neighbor_pool<T, decltype(csr)::value>), grid, block, 0, static_cast<hipStream_t>(stream),
                           (const T*)m->values, m->indptr, m->indices, m->ld, n, m->n_cols, g_indptr, g_indices,
                           (uint32_t)n_tiles, (int)shift, n_cells, out, ldo, flags);
    });
    HIP_TRY(hipGetLastError());
    return ICV_OK;
}

}  // extern "C"

// ---- the K-state model: tl.cnv_copy_states, tl.cnv_copy_posteriors, tl.cnv_copy_states_filter, tl.cnv_copy_states_fit
//  ------------------------------------------------------------------------------------------------
static_assert(icv::kCsMaxWindows == ICV_COPY_STATES_MAX_WINDOWS, "the header's window cap is the kernel's");
static_assert((size_t)icv::kCsMaxWindows * icv::kCsLdsPerWindow <= (size_t)icv::kLdsLimit, "one cell fits a CU's LDS");
static_assert(icv::kCpLdsBytes == ICV_COPY_POSTERIOR_LDS_BYTES && icv::kCpLdsBytes <= icv::kLdsLimit,
              "the header's LDS budget is the kernel's and one cell fits a CU's LDS");
static_assert(icv::cp_max_windows(2) == ICV_COPY_POSTERIOR_MAX_WINDOWS(2) &&
                  icv::cp_max_windows(icv::kCsMaxStates) == ICV_COPY_POSTERIOR_MAX_WINDOWS(icv::kCsMaxStates),
              "the header's window cap is the kernel's");
static_assert(ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(6, 1) == 2923 && ICV_COPY_POSTERIOR_STATS_LDS(2923, 6, 1) <= icv::kCpLdsBytes &&
                  ICV_COPY_POSTERIOR_STATS_LDS(2924, 6, 1) > icv::kCpLdsBytes,
              "the header's cap of icv_copy_posterior_stats is the largest n_cols whose LDS fits");

namespace {

// what is wrong with the model of icv_copy_states_viterbi, in the order it is reported; nullptr when nothing is
const char* cs_params_fault(const double* levels, int32_t n_levels, int32_t neutral, double h, double stay, double sw) {
    if (n_levels < 2 || n_levels > icv::kCsMaxStates) return "n_levels must lie in [2, 8]";
    if (neutral < 0 || neutral >= n_levels) return "neutral must be the index of a level";
    for (int32_t k = 0; k < n_levels; ++k)
        if (!std::isfinite(levels[k])) return "the levels must be finite";
    for (int32_t k = 1; k < n_levels; ++k)
        if (!(levels[k] > levels[k - 1])) return "the levels must ascend strictly";
    if (levels[neutral] != 0.0) return "levels[neutral] must be 0";
    if (!(std::isfinite(h) && h > 0.0 && std::isfinite(stay) && std::isfinite(sw)))
        return "h must be finite and > 0, stay and sw finite";
    return nullptr;
}

// what is wrong with the model of icv_copy_posterior_chains and icv_copy_posterior_stats, in the order it is reported: the
// model check of icv_copy_states_viterbi (its stay and sw have no part here), then these entries' own scalars
const char* cp_params_fault(const double* levels, int32_t n_levels, int32_t neutral, double h, double ps, double pw) {
    const char* fault = cs_params_fault(levels, n_levels, neutral, h, 0.0, 0.0);
    if (!fault && !(ps > 0.0 && ps < 1.0 && std::isnormal(pw) && pw > 0.0 && pw < 1.0))
        fault = "ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)";
    return fault;
}

// the checked model as the kernels take it; stay, sw: log(1 - p), log(p / (K - 1)) for Viterbi, ps, pw for forward-backward
icv::CsParams cs_params(const double* levels, int32_t n_levels, int32_t neutral, double h, double stay, double sw) {
    icv::CsParams P{};
    for (int32_t k = 0; k < n_levels; ++k) P.mu[k] = levels[k];
    P.mu[neutral] = 0.0;  // (a -0.0 is used as 0.0)
    P.h = h, P.stay = stay, P.sw = sw, P.z = neutral;
    return P;
}

// the K of a window cap and its message: an n_levels outside [2, 8] is the model's fault, which is reported after the cap
int cs_cap_states(int32_t n_levels) { return std::min(std::max(n_levels, 2), icv::kCsMaxStates); }

// One instantiation by the number of states (2 .. 8, checked by the caller): f, a generic lambda, gets
// std::integral_constant<int, K>.
template <typename F>
int by_states(int32_t n_levels, F&& f) {
    switch (n_levels) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

}  // namespace

extern "C" {

int icv_copy_states_viterbi(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, const double* levels,
                            int32_t n_levels, int32_t neutral, double h, double stay, double sw, int8_t* states,
                            int8_t* sign, int32_t* nonneutral, void* stream) {
    const char* fault = levels ? cs_params_fault(levels, n_levels, neutral, h, stay, sw) : nullptr;
    ICV_TRY(hmm_check("copy_states_viterbi", m, chr_start, n_chr, levels && states && sign && nonneutral,
                      ICV_COPY_STATES_MAX_WINDOWS, icv::kCsLdsPerWindow, fault == nullptr, fault ? fault : ""));
    const icv::CsParams P = cs_params(levels, n_levels, neutral, h, stay, sw);
    return by_states(n_levels, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return hmm_launch([](auto t, auto csr) { return icv::k_copy_states_viterbi<decltype(t), decltype(csr)::value, K>; }, m,
                          chr_start, n_chr, icv::cs_lds_bytes(m->n_cols), stream, P, states, sign, nonneutral);
    });
}

int icv_copy_posterior_chains(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, const double* levels,
                              int32_t n_levels, int32_t neutral, double h, double ps, double pw, double* neutral_out,
                              double* planes_out_or_null, void* stream) {
    const char* fault = levels ? cp_params_fault(levels, n_levels, neutral, h, ps, pw) : nullptr;
    const int kc = cs_cap_states(n_levels);
    ICV_TRY(hmm_check("copy_posterior_chains", m, chr_start, n_chr, levels && neutral_out, icv::cp_max_windows(kc),
                      8 * (kc + 1), fault == nullptr, fault ? fault : "", " with K = " + std::to_string(kc) + " states"));
    const icv::CsParams P = cs_params(levels, n_levels, neutral, h, ps, pw);
    return by_states(n_levels, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return hmm_launch([](auto t, auto csr) { return icv::k_copy_posterior_chains<decltype(t), decltype(csr)::value, K>; }, m,
                          chr_start, n_chr, icv::cp_lds_bytes(m->n_cols, K), stream, P, neutral_out, planes_out_or_null);
    });
}

// the E-step of the Baum-Welch fit of the K-state model
int icv_copy_posterior_stats(const icv_matrix* m, const int32_t* chr_start, int32_t n_chr, const double* levels,
                             int32_t n_levels, int32_t neutral, double h, double ps, double pw, double* stats,
                             void* stream) {
    const char* fault = levels ? cp_params_fault(levels, n_levels, neutral, h, ps, pw) : nullptr;
    const int kc = cs_cap_states(n_levels);
    ICV_TRY(hmm_check("copy_posterior_stats", m, chr_start, n_chr, levels && stats, icv::cps_max_windows(kc, n_chr),
                      8 * (kc + 1), fault == nullptr, fault ? fault : "",
                      " with K = " + std::to_string(kc) + " states, beside " + std::to_string(8 * (2 * kc + 1)) +
                          " bytes for each of the " + std::to_string(n_chr) + " chromosomes, of " +
                          std::to_string(icv::kCpLdsBytes) + " bytes"));
    const icv::CsParams P = cs_params(levels, n_levels, neutral, h, ps, pw);
    return by_states(n_levels, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return hmm_launch([](auto t, auto csr) { return icv::k_copy_posterior_stats<decltype(t), decltype(csr)::value, K>; }, m,
                          chr_start, n_chr, (size_t)icv::cps_lds_bytes(m->n_cols, K, n_chr), stream, P, stats);
    });
}

int icv_copy_states_filter(const int8_t* states, const double* p_neutral, int64_t n_rows, int32_t n_cols,
                           const int32_t* chr_start, int32_t n_chr, double max_p_normal, int8_t* filtered, int8_t* sign,
                           int32_t* nonneutral, int32_t* removed, int32_t* bad, void* stream) {
    if (seg_bad_shape(states, n_rows, n_cols, chr_start, n_chr) || !p_neutral || !filtered || !sign || !nonneutral ||
        !removed || !bad || !(max_p_normal >= 0.0 && max_p_normal <= 1.0))
        return fail(ICV_ERR_INVALID, "bad copy_states_filter arguments");
    return filter_launch("copy_states_filter", states, p_neutral, n_rows, n_cols, chr_start, n_chr, max_p_normal, filtered, sign,
                         nonneutral, removed, bad, stream);
}

}  // extern "C"
