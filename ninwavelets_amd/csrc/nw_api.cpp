// nw_api.cpp — the C ABI of libninwave.so (include/ninwave.h).
//
// Pipeline per device chunk of signals:
//   x (S, n) --H2D/D2D--> d_x --rocFFT R2C--> d_X (S, n/2+1)
//   engine ROCFFT: K1 multiply -> d_Y (S, F, n) -> rocFFT C2C inverse in place -> K2 epilogue
//   engine FUSED : one kernel: W*X -> LDS Stockham inverse FFT -> epilogue store
// The wavelet is never materialised on the host: analytic kinds are evaluated
// inside the kernels from (kind, params, freqs, grid).
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "nw_dcheck.h"
#include "nw_internal.h"

namespace {

thread_local std::string g_last_error;

// NW_LOG (SURVEY.md §5 "Metrics / logging"; the reference only prints SizeError, base.py:71-72):
// 0 = silent (default), 1 = plan / engine / reduction-path decisions and every error status,
// 2 = also every launch stage with its kernel and, under NW_TIMING, its time.  Read from the
// environment at first use; nw_set_log_level() overrides it.  One line per event on stderr.
std::atomic<int> g_log_level{-1};
std::mutex g_log_mu;

int log_level() {
    int l = g_log_level.load(std::memory_order_relaxed);
    if (l >= 0) return l;
    const char* s = std::getenv("NW_LOG");
    int expect = -1;
    g_log_level.compare_exchange_strong(expect, s ? std::max(0, std::atoi(s)) : 0);
    return g_log_level.load();
}

__attribute__((format(printf, 2, 3))) void nw_logf(int level, const char* fmt, ...) {
    if (log_level() < level) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> g(g_log_mu);
    std::fprintf(stderr, "[ninwave] %s\n", buf);
}

const char* out_name(int k) {
    static const char* names[] = {"cwt", "abs", "power", "power_mean", "itc", "power_sum", "phase_sum",
                                  "cross_sum", "plv_sum", "lag_sum"};
    if (k == 1001) return "power partials";
    if (k == 1002) return "phase partials";
    if (k == 1003) return "cross partials";
    if (k == 1004) return "plv partials";
    return k >= 0 && k < 10 ? names[k] : "?";
}
const char* kernel_name(int64_t k) {
    static const char* names[] = {"none", "nw_fused_kernel", "nw_fused_pair_kernel", "nw_chirp_kernel",
                                  "rows_kernel + cols_kernel", "k1_multiply + rocFFT", "nw_fused_decim_kernel"};
    return k >= 0 && k < 7 ? names[k] : "?";
}
const char* dtype_name(int dt) { return dt == NW_F32 ? "float32" : "float64"; }

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    nw_logf(1, "error %d: %s", code, msg.c_str());
    return code;
}

#define NW_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? NW_E_NOMEM : NW_E_HIP,                    \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

#define NW_RF(expr)                                                                           \
    do {                                                                                      \
        rocfft_status s_ = (expr);                                                            \
        if (s_ != rocfft_status_success)                                                      \
            return fail(NW_E_ROCFFT, std::string(#expr) + ": rocfft status " + std::to_string((int)s_)); \
    } while (0)

#define NW_TRY(expr)                 \
    do {                             \
        int r_ = (expr);             \
        if (r_ != NW_OK) return r_;  \
    } while (0)

std::once_flag g_rocfft_once;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// debug library: every kernel file's check words (nw_dcheck.h), read and cleared after each
// synchronising call; the product library registers none
std::vector<nw::DcheckTake>& dcheck_registry() {
    static std::vector<nw::DcheckTake> r;
    return r;
}

#ifdef NW_DEBUG_BOUNDS
constexpr bool kDebugBounds = true;
#else
constexpr bool kDebugBounds = false;
#endif

// after the device's work is complete: NW_E_BOUNDS if any kernel check failed since the last call
int dcheck_collect(hipStream_t stream) {
    if (!kDebugBounds) return NW_OK;
    hipError_t e = stream ? hipStreamSynchronize(stream) : hipDeviceSynchronize();
    if (e != hipSuccess) return fail(NW_E_HIP, std::string("synchronize: ") + hipGetErrorString(e));
    std::string msg;
    for (nw::DcheckTake take : dcheck_registry()) {
        unsigned fails = 0, site = 0;
        const char* file = "";
        e = take(&fails, &site, &file);
        if (e != hipSuccess) return fail(NW_E_HIP, std::string("bounds-check readback: ") + hipGetErrorString(e));
        if (!fails) continue;
        std::string where = site >= nw::kDcheckReduceSite
                                ? "nw_reduce_dev.h:" + std::to_string(site - nw::kDcheckReduceSite)
                                : site >= nw::kDcheckHeaderSite
                                      ? "nw_fft_dev.h:" + std::to_string(site - nw::kDcheckHeaderSite)
                                      : std::string(file) + ":" + std::to_string(site);
        msg += (msg.empty() ? "" : "; ") + std::to_string(fails) + " failing check(s), first at " + where;
    }
    return msg.empty() ? NW_OK : fail(NW_E_BOUNDS, "kernel bounds check: " + msg);
}

// Device memory that frees itself.  ensure() grows only: a buffer at least `want` long stays.
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr, o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(ptr, o.ptr);
            std::swap(bytes, o.bytes);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    int ensure(size_t want) {
        if (bytes >= want && ptr) return NW_OK;
        if (ptr) {
            NW_HIP(hipFree(ptr));
            ptr = nullptr;
            bytes = 0;
        }
        NW_HIP(hipMalloc(&ptr, want));
        bytes = want;
        return NW_OK;
    }
    void reset() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    char* at(size_t off) const { return (char*)ptr + off; }
};

// a rocFFT plan / execution info of one scope
struct ScopedFftPlan {
    rocfft_plan h = nullptr;
    ~ScopedFftPlan() {
        if (h) rocfft_plan_destroy(h);
    }
};
struct ScopedFftInfo {
    rocfft_execution_info h = nullptr;
    ~ScopedFftInfo() {
        if (h) rocfft_execution_info_destroy(h);
    }
};

enum Stage { ST_FWD = 0, ST_MUL, ST_INV, ST_EPI, ST_FUSED, ST_COPY, ST_ROWS, ST_EXPAND, ST_N };
const char* const kStageName[ST_N] = {"forward", "multiply", "inverse", "epilogue", "fused", "copy", "rows", "expand"};

struct Pending {
    int stage;
    hipEvent_t a, b;
    bool own_a = true;   // false: a is the previous stage's b (chained), released with it
};

// How a plan transforms a chunk: rocFFT forward / K1 multiply / rocFFT inverse / K2 epilogue, or
// one of the three fused forms: one-pass (power-of-two n <= 16384, nw_fused.hip), two-pass
// (longer powers of two, nw_large.hip), chirp-z (other n, nw_chirp.hip).
enum Form { FORM_ROCFFT, FORM_ONE_PASS, FORM_TWO_PASS, FORM_CHIRP };

// Some rows of a wavelet seen as a wavelet of their own: the compacted per-row arrays (and table
// rows) of desc, and the map that scatters the U computed rows to their scales (k_expand_rows:
// row u goes to the scales order[offs[u] .. offs[u + 1])).  U == 0: no view.
struct RowView {
    nw::WDesc desc{};
    DevBuf buf;      // nw::host::row_view_layout
    int U = 0;
    const int32_t* offs = nullptr;
    const int32_t* order = nullptr;
    void reset() {
        buf.reset();
        U = 0;
        offs = order = nullptr;
    }
};

}  // namespace

struct nw_plan {
    int device = 0;
    int64_t n = 0, nh = 0, max_batch = 0;
    int nfreq = 0, dtype = NW_F32;
    // time decimation (nw_plan_set_decim): every output row holds the n / decim samples
    // y[0], y[decim], ... of the full row; fixed before the first execute
    int decim = 1;
    bool executed = false;
    int64_t n_out() const { return n / decim; }
    uint32_t flags = 0;
    Form form = FORM_ROCFFT;
    // auto engine, chirp-z length with 2n - 1 > M_max: chirp-z only if some row's support fits
    // (checked when the table is built); if none does, form is FORM_ROCFFT until the next
    // nw_plan_set_wavelet
    bool chirp_tentative = false;
    size_t esz = 4;  // real element size

    hipStream_t own_stream = nullptr, stream = nullptr;

    // wavelet
    bool has_wavelet = false;
    nw::WDesc desc{};
    DevBuf d_freq, d_peak, d_xstep32, d_table, d_row_len;
    std::vector<int64_t> row_len_host;   // tables: true length of each row

    // repeated rows: when at most half the F rows of W are distinct (Shannon ignores f,
    // wavelets.py:256-262; repeated freqs), the engines run on the view of the U distinct rows
    // into d_uout and k_expand_rows copies each computed row to every scale that repeats it
    // (the view's map: the scales grouped by distinct row).  NW_NO_DEDUP turns it off.
    RowView uniq;
    DevBuf d_uout;

    // buffers
    DevBuf d_x, d_X;
    DevBuf d_Y;
    DevBuf d_out;
    DevBuf d_acc;                    // epoch reductions: fp64 (F, n) sums (x2 for phases); nw_execute_conn:
                                     // complex (npairs, F, n) | (nchan, F, n) | the pair tiles
    std::vector<nw::ConnTile> conn_tiles;   // nw_execute_conn: the last call's tiles (the upload's source)
    std::vector<int32_t> pac_lists;         // nw_execute_pac, _pac_bins, _erpac: the last call's ip | ia | fph | fam (likewise)
    DevBuf d_pstage;                 // nw_execute_pac_surr: one chunk's staged unit phasors and magnitudes, then its
                                     // per-channel sums where the caller gave no buffer for them
    // nw_execute_multi_device reductions: this device's fp64 partial sums, and (device 0's
    // plan) the peer-copy landing buffer; kept across calls (a hipFree per call would
    // synchronise the device on every epoch-loop iteration)
    DevBuf d_part, d_gather;
    DevBuf d_wtab;                   // fused engine: W[f, k] (pad_to + 1/n applied); n > 16384: kmax[f]
    bool wtab_valid = false;
    int64_t chirp_counts[5] = {0, 0, 0, 0, 0};   // rows per M class (M = 1024 << c)
    // execute_reduce, chirp-z partial sums: the chunk being run continues the signal group of the
    // one before it, whose partial row the kernel adds to (chirp_psum_chunk, nw_shape.h)
    bool chirp_carry = false;
    // execute_reduce, one-pass partial sums: the chunk being run lies inside a signal group, so the
    // kernel leaves one fp64 row per signal (the terms) and execute_reduce adds them as a block would
    bool psum_per_signal = false;
    // chirp-z rows of a tentative length wider than the largest on-chip transform: computed
    // by the rocFFT path on a view of just those rows into d_oscr and scattered to their
    // scales (k_expand_rows), the other rows stay on chip
    RowView over;
    DevBuf d_oscr;
    DevBuf d_scratch;                // two-pass form: Xt + B

    // rocFFT, keyed by batch count
    std::map<int64_t, rocfft_plan> fwd, inv;
    rocfft_execution_info info = nullptr;
    DevBuf work;

    // host-buffer output: two pinned staging pieces (the DMA of piece i overlaps the
    // host copy of piece i-1 into the caller's pageable array)
    void* pinned[2] = {nullptr, nullptr};
    hipEvent_t pinned_ev[2] = {nullptr, nullptr};

    // timing
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    nw_stats stats{};

    // the sized buffers nw_stats.device_bytes counts (the per-freq arrays, row views and rocFFT
    // plan objects are small)
    size_t device_bytes() const {
        size_t sum = 0;
        for (const DevBuf* b : {&d_x, &d_X, &d_table, &d_uout, &d_Y, &d_out, &d_acc, &d_part, &d_gather, &d_wtab,
                                &d_oscr, &d_scratch, &d_pstage, &work})
            sum += b->bytes;
        return sum;
    }

    nw_plan() = default;
    nw_plan(const nw_plan&) = delete;
    nw_plan& operator=(const nw_plan&) = delete;
    // on the plan's device (nw_plan_destroy, nw_plan_create); the DevBufs free themselves
    ~nw_plan() {
        for (auto& kv : fwd) rocfft_plan_destroy(kv.second);
        for (auto& kv : inv) rocfft_plan_destroy(kv.second);
        if (info) rocfft_execution_info_destroy(info);
        for (const Pending& pe : pending) {
            if (pe.own_a) (void)hipEventDestroy(pe.a);
            (void)hipEventDestroy(pe.b);
        }
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        for (int i = 0; i < 2; ++i) {
            if (pinned[i]) (void)hipHostFree(pinned[i]);
            if (pinned_ev[i]) (void)hipEventDestroy(pinned_ev[i]);
        }
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

nw::StageEvents& nw::stage_events() {
    static thread_local StageEvents se;
    return se;
}

namespace {

int take_event(nw_plan* p, hipEvent_t* ev) {
    if (!p->event_pool.empty()) {
        *ev = p->event_pool.back();
        p->event_pool.pop_back();
        return NW_OK;
    }
    // timing only (resolve_timing synchronises the stream before reading them): no system-scope
    // fence at record, whose L2 writeback + invalidate between a step's two launches cost C2
    // (one 0.23 ms launch per step) 0.04 ms per step and showed up in the stage times
    NW_HIP(hipEventCreateWithFlags(ev, hipEventDisableSystemFence));
    return NW_OK;
}

// launch counts are kept with or without NW_TIMING (they tell which kernels ran)
void count_launch(nw_plan* p, int stage) {
    switch (stage) {
        case ST_MUL: p->stats.launches_multiply++; break;
        case ST_FUSED: p->stats.launches_fused++; break;
        case ST_ROWS: p->stats.launches_rows++; break;
        case ST_EXPAND: p->stats.launches_expand++; break;
        default: break;
    }
}

// Run `fn` on the plan stream as one stage: counted, logged and, when NW_TIMING is set, timed by
// two events.
// kernels = false: the events are markers recorded around fn (rocFFT, copies).
// kernels = true: fn's work is kernels launched through nw_launch (nw_internal.h) and the events
// ride on those launches (hipExtLaunchKernel: the stop event is the last dispatch's own end; the
// start event is one marker before the first), so a chained stage adds no marker at all; a stage
// that launched nothing records both at once (0 ms).
// chain = true: the caller enqueued nothing on the stream since the previous stage returned, so
// that stage's end event is this one's start (one event record less per boundary: each costs the
// stream a few microseconds, 3 % of a C2 step).  NW_TIMING_CHAIN chains every stage.
template <typename F>
int run_stage(nw_plan* p, int stage, bool kernels, bool chain, F&& fn) {
    count_launch(p, stage);
    nw_logf(2, "plan %p: launch %s%s%s", (void*)p, kStageName[stage], stage == ST_FUSED || stage == ST_ROWS ? ": " : "",
            stage == ST_FUSED || stage == ST_ROWS ? kernel_name(p->stats.kernel) : "");
    if (!(p->flags & NW_TIMING)) return fn();
    Pending pe{stage, nullptr, nullptr};
    const bool chained = (chain || (p->flags & NW_TIMING_CHAIN)) && !p->pending.empty();
    if (chained) {
        pe.a = p->pending.back().b;
        pe.own_a = false;
    } else {
        NW_TRY(take_event(p, &pe.a));
        if (!kernels) NW_HIP(hipEventRecord(pe.a, p->stream));
    }
    NW_TRY(take_event(p, &pe.b));
    nw::StageEvents& se = nw::stage_events();
    if (kernels) se = nw::StageEvents{chained ? nullptr : pe.a, pe.b, 0};
    const int r = fn();
    const bool stamped = se.launches > 0;   // the launches took the events
    se = nw::StageEvents{};
    if (kernels && !stamped && !chained) NW_HIP(hipEventRecord(pe.a, p->stream));
    if (!stamped) NW_HIP(hipEventRecord(pe.b, p->stream));
    p->pending.push_back(pe);
    return r;
}

template <typename F>
int staged(nw_plan* p, int stage, F&& fn) {
    return run_stage(p, stage, false, false, fn);
}

// a stage that is one kernel launcher call (its text names the call in an error message)
#define NW_KERNEL_STAGE(p, stage, chain, call) \
    run_stage(p, stage, true, chain, [&] {     \
        NW_HIP(call);                          \
        return NW_OK;                          \
    })

int resolve_timing(nw_plan* p) {
    if (p->pending.empty()) return NW_OK;
    NW_HIP(hipStreamSynchronize(p->stream));
    for (const Pending& pe : p->pending) {
        float ms = 0.f;
        NW_HIP(hipEventElapsedTime(&ms, pe.a, pe.b));
        nw_logf(2, "plan %p: %s %.3f ms", (void*)p, kStageName[pe.stage], ms);
        switch (pe.stage) {
            case ST_FWD: p->stats.ms_forward += ms; break;
            case ST_MUL: p->stats.ms_multiply += ms; break;
            case ST_INV: p->stats.ms_inverse += ms; break;
            case ST_EPI: p->stats.ms_epilogue += ms; break;
            case ST_FUSED: p->stats.ms_fused += ms; break;
            case ST_ROWS: p->stats.ms_rows += ms; break;
            case ST_EXPAND: p->stats.ms_expand += ms; break;
            default: p->stats.ms_copy += ms; break;
        }
        if (pe.own_a) p->event_pool.push_back(pe.a);
        p->event_pool.push_back(pe.b);
    }
    p->pending.clear();
    return NW_OK;
}

// `d` (the plan's wavelet or a view of it) with the execute-time geometry: pad_to the cached
// rows to n, mask X (base.py:396-401)
nw::WDesc with_geometry(const nw_plan* p, nw::WDesc d) {
    d.n = p->n;
    d.nh = p->nh;
    d.scale = 1.0 / (double)p->n;
    d.off = d.len_full < p->n ? (p->n - d.len_full) / 2 : 0;
    d.xlim = (p->flags & NW_INTERPOLATE) ? p->n / 2 : p->n;   // int(n / 2) (base.py:120)
    return d;
}

rocfft_precision prec(const nw_plan* p) {
    return p->dtype == NW_F32 ? rocfft_precision_single : rocfft_precision_double;
}

// rocFFT plans keyed by batch count: R2C forward over signals, C2C inverse (in place)
// over (signal, scale) rows.
int get_plan(nw_plan* p, bool inverse, int64_t batch, rocfft_plan* out) {
    auto& m = inverse ? p->inv : p->fwd;
    auto it = m.find(batch);
    if (it == m.end()) {
        size_t len = (size_t)p->n;
        rocfft_plan pl = nullptr;
        NW_RF(rocfft_plan_create(&pl, inverse ? rocfft_placement_inplace : rocfft_placement_notinplace,
                                 inverse ? rocfft_transform_type_complex_inverse : rocfft_transform_type_real_forward,
                                 prec(p), 1, &len, (size_t)batch, nullptr));
        m[batch] = pl;
        size_t ws = 0;
        NW_RF(rocfft_plan_get_work_buffer_size(pl, &ws));
        if (ws > p->work.bytes) NW_TRY(p->work.ensure(ws));
        it = m.find(batch);
    }
    *out = it->second;
    return NW_OK;
}

// One rocFFT execution covers at most 2^31 elements: a single 512 x 2^24 batch
// (C5, 8.6e9 elements) completes only part of its rows, so longer batches run as
// several executions of <= kFftElems / n rows each.
constexpr int64_t kFftElems = int64_t(1) << 31;

int run_fft(nw_plan* p, rocfft_plan plan, void* in, void* out) {
    NW_RF(rocfft_execution_info_set_stream(p->info, p->stream));
    if (p->work.bytes) NW_RF(rocfft_execution_info_set_work_buffer(p->info, p->work.ptr, p->work.bytes));
    void* ib[1] = {in};
    void* ob[1] = {out};
    NW_RF(rocfft_execute(plan, ib, out ? ob : nullptr, p->info));
    return NW_OK;
}

// The rocFFT engine's Y buffer (max_batch x nfreq x n complex) is allocated on first need:
// a device-output CWT writes Y straight into the caller's buffer and never needs it
// (at C5, 512 x 2^24 complex64 = 68.7 GB of HBM saved).
int need_Y(nw_plan* p, int nfreq) { return p->d_Y.ensure((size_t)p->max_batch * nfreq * p->n * 2 * p->esz); }

// rows transforms of length n starting at in/out (elem bytes per input / output element)
int run_fft_rows(nw_plan* p, bool inverse, int64_t rows, char* in, char* out, size_t in_row, size_t out_row) {
    const int64_t group = std::max<int64_t>(1, kFftElems / p->n);
    for (int64_t r0 = 0; r0 < rows; r0 += group) {
        const int64_t nb = std::min<int64_t>(group, rows - r0);
        rocfft_plan pl = nullptr;
        NW_TRY(get_plan(p, inverse, nb, &pl));
        NW_TRY(run_fft(p, pl, in + r0 * in_row, out ? out + r0 * out_row : nullptr));
    }
    return NW_OK;
}

// One batched in-place fp64 C2C rocFFT per distinct row length: by_len maps a length to its
// rows, which lie consecutively in buf (complex fp64) from the first one's rows[].off.
template <typename Row>
int fft_rows_by_length(const std::vector<Row>& rows, const std::map<int64_t, std::vector<int>>& by_len, bool inverse,
                       void* buf, hipStream_t stream) {
    ScopedFftInfo info;
    NW_RF(rocfft_execution_info_create(&info.h));
    if (stream) NW_RF(rocfft_execution_info_set_stream(info.h, stream));
    for (const auto& kv : by_len) {
        if (kv.first == 0) continue;
        ScopedFftPlan pl;
        size_t len = (size_t)kv.first, ws = 0;
        NW_RF(rocfft_plan_create(&pl.h, rocfft_placement_inplace,
                                 inverse ? rocfft_transform_type_complex_inverse : rocfft_transform_type_complex_forward,
                                 rocfft_precision_double, 1, &len, kv.second.size(), nullptr));
        NW_RF(rocfft_plan_get_work_buffer_size(pl.h, &ws));
        DevBuf work;
        if (ws) {
            NW_TRY(work.ensure(ws));
            NW_RF(rocfft_execution_info_set_work_buffer(info.h, work.ptr, ws));
        }
        void* ib[1] = {(char*)buf + (size_t)rows[kv.second[0]].off * 2 * sizeof(double)};
        NW_RF(rocfft_execute(pl.h, ib, nullptr, info.h));
        NW_HIP(stream ? hipStreamSynchronize(stream) : hipDeviceSynchronize());
    }
    return NW_OK;
}

// The view of the rows `rows` of d (gathered on the device: launch_gather copies bits) with the
// scatter map `map` = offs[U + 1] then order[].
int build_row_view(nw_plan* p, const nw::WDesc& d, const std::vector<int>& rows, const std::vector<int32_t>& map,
                   RowView* v) {
    const int U = (int)rows.size();
    const bool table = d.kind == NW_TABLE;
    const size_t trow = table ? (size_t)d.len_full * 2 * p->esz : 0;
    const nw::host::RowViewLayout l = nw::host::row_view_layout(U, map.size() - (size_t)(U + 1), trow);
    v->reset();
    NW_TRY(v->buf.ensure(l.bytes));
    std::vector<int32_t> head(l.freq / 4, 0);
    std::copy(rows.begin(), rows.end(), head.begin() + l.idx / 4);
    std::copy(map.begin(), map.begin() + U + 1, head.begin() + l.offs / 4);
    std::copy(map.begin() + U + 1, map.end(), head.begin() + l.order / 4);
    NW_HIP(hipMemcpy(v->buf.ptr, head.data(), l.freq, hipMemcpyHostToDevice));
    const int32_t* idx = (const int32_t*)v->buf.at(l.idx);
    nw::WDesc o = d;
    o.nfreq = U;
    if (d.freq) {
        NW_HIP(nw::launch_gather(d.freq, v->buf.at(l.freq), idx, U, 8, p->stream));
        o.freq = (const double*)v->buf.at(l.freq);
    }
    if (d.peak) {
        NW_HIP(nw::launch_gather(d.peak, v->buf.at(l.peak), idx, U, 8, p->stream));
        o.peak = (const double*)v->buf.at(l.peak);
    }
    if (d.xstep32) {
        NW_HIP(nw::launch_gather(d.xstep32, v->buf.at(l.xstep), idx, U, 4, p->stream));
        o.xstep32 = (const float*)v->buf.at(l.xstep);
    }
    if (table && d.row_len) {
        NW_HIP(nw::launch_gather(d.row_len, v->buf.at(l.row_len), idx, U, 8, p->stream));
        o.row_len = (const int64_t*)v->buf.at(l.row_len);
    }
    if (table && trow) {
        NW_HIP(nw::launch_gather(d.table, v->buf.at(l.table), idx, U, trow, p->stream));
        o.table = v->buf.at(l.table);
    }
    NW_HIP(hipStreamSynchronize(p->stream));
    v->desc = o;
    v->offs = (const int32_t*)v->buf.at(l.offs);
    v->order = (const int32_t*)v->buf.at(l.order);
    v->U = U;
    return NW_OK;
}

// The chirp-z table (W rows, supports, rows grouped by M) of the rows of d.  A tentative length
// (2n - 1 > M_max) none of whose rows fit switches the plan to the rocFFT form until the next
// nw_plan_set_wavelet; if only some do not fit, those get the overflow view (offs = 0 .. U,
// order = the rows).
int chirp_table(nw_plan* p, const nw::WDesc& d) {
    if (p->wtab_valid) return NW_OK;
    NW_TRY(p->d_wtab.ensure(nw::chirp_wtable_bytes(p->n, d.nfreq, p->dtype, d.kind)));
    bool fits = true;
    std::vector<int> over;
    p->over.reset();
    NW_HIP(nw::build_chirp_wtable(d, p->dtype, p->d_wtab.ptr, p->stream, p->chirp_counts, &fits, &over));
    if (!fits) {
        if (!p->chirp_tentative)
            return fail(NW_E_INVALID, "chirp-z form: a wavelet row is wider than the largest on-chip transform");
        if ((int)over.size() >= d.nfreq) {   // no row fits: the rocFFT engine
            p->form = FORM_ROCFFT;
            nw_logf(1, "plan %p: no wavelet row fits the on-chip chirp-z transform: rocFFT engine", (void*)p);
            return NW_OK;
        }
        std::vector<int32_t> map(over.size() + 1);
        for (size_t u = 0; u < map.size(); ++u) map[u] = (int32_t)u;
        map.insert(map.end(), over.begin(), over.end());
        NW_TRY(build_row_view(p, d, over, map, &p->over));
        nw_logf(1, "plan %p: chirp-z form, %d of %d rows too wide for the chip run through rocFFT (hybrid)",
                (void*)p, (int)over.size(), d.nfreq);
    }
    p->wtab_valid = true;
    return NW_OK;
}

constexpr int OUT_PSUM = 1001;    // internal run_chunk kinds: (ceil(c / 8), F, n) fp64 power partials,
constexpr int OUT_PHSUM = 1002;   // complex fp64 phase partials (y / |y|)
constexpr int OUT_XSUM = 1003;    // pair reductions: (ceil(c / 8), F, n, 4) fp64 cross partials of c interleaved
constexpr int OUT_PLVSUM = 1004;  // signals, (.., 2) unit-phasor product partials

// ---- one device chunk on the rows of d: xs (device, c signals) -> dst (device, (c, d.nfreq, n))

// forward R2C by rocFFT, which may use its input as scratch: transform from the plan's own copy
int forward_rocfft(nw_plan* p, const void* xs_dev, int64_t c) {
    if (xs_dev != p->d_x.ptr)
        NW_TRY(staged(p, ST_COPY, [&] {
            NW_HIP(hipMemcpyAsync(p->d_x.ptr, xs_dev, (size_t)c * p->n * p->esz, hipMemcpyDeviceToDevice, p->stream));
            return NW_OK;
        }));
    return staged(p, ST_FWD, [&] {
        return run_fft_rows(p, false, c, p->d_x.at(0), p->d_X.at(0), (size_t)p->n * p->esz, (size_t)p->nh * 2 * p->esz);
    });
}

// K1 multiply into Y, in-place C2C inverse; the complex rows are left in Y
int multiply_inverse(nw_plan* p, const nw::WDesc& d, int64_t c, void* Y) {
    NW_TRY(NW_KERNEL_STAGE(p, ST_MUL, false, nw::launch_multiply(d, p->dtype, p->d_X.ptr, Y, c, p->stream)));
    const size_t row = (size_t)p->n * 2 * p->esz;
    return staged(p, ST_INV, [&] { return run_fft_rows(p, true, c * d.nfreq, (char*)Y, nullptr, row, row); });
}

int run_rocfft(nw_plan* p, const nw::WDesc& d, const void* xs_dev, int64_t c, void* dst, int out_kind,
               bool dst_is_final) {
    NW_TRY(forward_rocfft(p, xs_dev, c));
    // K1 writes the product straight into the destination when the caller wants
    // the complex CWT on the device; otherwise into the plan's Y buffer.
    void* Y = dst;
    if (!(out_kind == NW_OUT_CWT && dst_is_final)) {
        NW_TRY(need_Y(p, d.nfreq));
        Y = p->d_Y.ptr;
    }
    p->stats.kernel = NW_K_MULTIPLY;
    NW_TRY(multiply_inverse(p, d, c, Y));
    if (out_kind == NW_OUT_CWT) {
        if (Y != dst)
            NW_TRY(staged(p, ST_COPY, [&] {
                NW_HIP(hipMemcpyAsync(dst, Y, (size_t)c * d.nfreq * p->n * 2 * p->esz, hipMemcpyDeviceToDevice,
                                      p->stream));
                return NW_OK;
            }));
        return NW_OK;
    }
    return NW_KERNEL_STAGE(p, ST_EPI, false,
                           nw::launch_epilogue(p->dtype, out_kind, Y, dst, c * d.nfreq * p->n, p->stream));
}

// one-pass form (power-of-two n <= 16384): the on-chip forward transform (nw_fused.hip's
// fwd_r2c_kernel: no copy, one kernel) reads the caller's rows directly
int run_one_pass(nw_plan* p, const nw::WDesc& d, const void* xs_dev, int64_t c, void* dst, int out_kind) {
    const bool table_was_valid = p->wtab_valid;
    NW_TRY(NW_KERNEL_STAGE(p, ST_FWD, false, nw::fused_forward(p->n, p->dtype, xs_dev, p->d_X.ptr, c, p->nh, p->stream)));
    if (!p->wtab_valid) {
        NW_TRY(p->d_wtab.ensure(nw::fused_wtable_bytes(p->n, d.nfreq, p->dtype, d.kind)));
        NW_HIP(nw::build_wtable(d, p->dtype, p->d_wtab.ptr, p->stream));
        p->wtab_valid = true;
    }
    if (out_kind == OUT_PSUM || out_kind == OUT_PHSUM) {
        p->stats.kernel = nw::fused_psum_kernel_id(p->n, p->dtype, out_kind == OUT_PHSUM);
        return NW_KERNEL_STAGE(p, ST_FUSED, false,
                               nw::fused_power_partials(d, p->dtype, out_kind == OUT_PHSUM, p->d_X.ptr, p->d_wtab.ptr,
                                                        dst, c, p->psum_per_signal, p->stream));
    }
    if (out_kind == OUT_XSUM || out_kind == OUT_PLVSUM) {
        p->stats.kernel = NW_K_FUSED_PAIR;
        return NW_KERNEL_STAGE(p, ST_FUSED, false,
                               nw::fused_pair_partials(d, p->dtype, out_kind == OUT_PLVSUM, p->d_X.ptr, p->d_wtab.ptr, dst,
                                                       c, p->stream));
    }
    if (p->decim > 1) {
        p->stats.kernel = NW_K_FUSED_DECIM;
        return NW_KERNEL_STAGE(p, ST_FUSED, table_was_valid,
                               nw::launch_fused_decim(d, p->dtype, out_kind, p->decim, p->d_X.ptr, p->d_wtab.ptr, dst, c,
                                                      p->stream));
    }
    p->stats.kernel = nw::fused_kernel_id(p->n, p->dtype, d.kind);
    // the forward stage was the last thing enqueued unless the table was built after it
    return NW_KERNEL_STAGE(p, ST_FUSED, table_was_valid,
                           nw::launch_fused(d, p->dtype, out_kind, p->d_X.ptr, p->d_wtab.ptr, dst, c, p->stream));
}

// two-pass form (n > 16384): per signal, X -> Xt, then per chunk of scales the row pass
// (W * X, length-N2 FFTs) into B and the column pass (length-N1 FFTs + epilogue) into the
// destination rows
int run_two_pass(nw_plan* p, const nw::WDesc& d, const void* xs_dev, int64_t c, void* dst, int out_kind) {
    NW_TRY(forward_rocfft(p, xs_dev, c));
    if (!p->wtab_valid) {
        NW_TRY(p->d_wtab.ensure(nw::large_support_bytes(d.nfreq)));
        NW_HIP(nw::build_large_support(d, p->dtype, p->d_wtab.ptr, p->stream));
        p->wtab_valid = true;
    }
    NW_TRY(p->d_scratch.ensure(nw::large_scratch_bytes(p->n, d.nfreq, p->dtype)));
    const size_t out_row = (size_t)p->n * (out_kind == NW_OUT_CWT ? 2 : 1) * p->esz;
    const int64_t fc = nw::large_fchunk(p->n, d.nfreq, p->dtype);
    void* const support = p->d_wtab.ptr;
    void* const scratch = p->d_scratch.ptr;
    p->stats.kernel = NW_K_TWO_PASS;
    for (int64_t sidx = 0; sidx < c; ++sidx) {
        const char* Xs = p->d_X.at((size_t)sidx * p->nh * 2 * p->esz);
        char* os = (char*)dst + (size_t)sidx * d.nfreq * out_row;
        // the spectrum transpose: timed with the copies
        NW_TRY(NW_KERNEL_STAGE(p, ST_COPY, false, nw::large_transpose(d, p->dtype, Xs, scratch, p->stream)));
        for (int64_t f0 = 0; f0 < d.nfreq; f0 += fc) {
            const int nf = (int)std::min<int64_t>(fc, d.nfreq - f0);
            NW_TRY(NW_KERNEL_STAGE(p, ST_ROWS, true,
                                   nw::large_rows(d, p->dtype, (int)f0, nf, support, scratch, p->stream)));
            NW_TRY(NW_KERNEL_STAGE(p, ST_FUSED, true,
                                   nw::large_cols(d, p->dtype, out_kind, (int)f0, nf, support, scratch, os, p->stream)));
        }
    }
    return NW_OK;
}

// The overflow rows of a hybrid chirp-z plan through the rocFFT path (K1 on their view,
// in-place C2C inverse, epilogue), then scattered to their scales of dst (nf of them).
int run_overflow_rows(nw_plan* p, int nf, int64_t c, void* dst, int out_kind) {
    const int U = p->over.U;
    const nw::WDesc od = with_geometry(p, p->over.desc);
    const size_t crow = (size_t)p->n * 2 * p->esz;
    const size_t orow = (size_t)p->n * (out_kind == NW_OUT_CWT ? 2 : 1) * p->esz;
    const size_t ybytes = (size_t)c * U * crow;
    NW_TRY(p->d_oscr.ensure(ybytes + (out_kind == NW_OUT_CWT ? 0 : (size_t)c * U * orow)));
    char* Y = p->d_oscr.at(0);
    NW_TRY(multiply_inverse(p, od, c, Y));
    const char* src = Y;
    if (out_kind != NW_OUT_CWT) {
        char* Z = Y + ybytes;
        NW_TRY(NW_KERNEL_STAGE(p, ST_EPI, false, nw::launch_epilogue(p->dtype, out_kind, Y, Z, c * U * p->n, p->stream)));
        src = Z;
    }
    return NW_KERNEL_STAGE(p, ST_EXPAND, false,
                           nw::launch_expand_rows(src, dst, c, U, nf, orow, p->over.offs, p->over.order, p->stream));
}

// chirp-z form (any other n up to 8192 fp32 / 4096 fp64): two on-chip FFTs per row.  A tentative
// length was settled by nw_execute, so the table leaves the form as it is.
int run_chirp(nw_plan* p, const nw::WDesc& d, const void* xs_dev, int64_t c, void* dst, int out_kind) {
    NW_TRY(forward_rocfft(p, xs_dev, c));
    NW_TRY(chirp_table(p, d));
    p->stats.kernel = NW_K_CHIRP;
    NW_TRY(NW_KERNEL_STAGE(p, ST_FUSED, false,
                           nw::launch_chirp(d, p->dtype, out_kind, p->d_X.ptr, p->d_wtab.ptr, dst, c, p->chirp_counts,
                                            p->chirp_carry, p->stream)));
    // launches_fused counts kernel launches: launch_chirp made one per M class that holds rows,
    // the stage counted one
    int64_t classes = 0;
    for (int64_t cnt : p->chirp_counts) classes += cnt != 0;
    if (classes > 1) p->stats.launches_fused += classes - 1;
    return p->over.U ? run_overflow_rows(p, d.nfreq, c, dst, out_kind) : NW_OK;
}

int run_chunk_rows(nw_plan* p, const nw::WDesc& d, const void* xs_dev, int64_t c, void* dst, int out_kind,
                   bool dst_is_final) {
    switch (p->form) {
        case FORM_ONE_PASS: return run_one_pass(p, d, xs_dev, c, dst, out_kind);
        case FORM_TWO_PASS: return run_two_pass(p, d, xs_dev, c, dst, out_kind);
        case FORM_CHIRP: return run_chirp(p, d, xs_dev, c, dst, out_kind);
        default: return run_rocfft(p, d, xs_dev, c, dst, out_kind, dst_is_final);
    }
}

// The rows an execute transforms: the view of the distinct rows if there is one, else every row.
nw::WDesc exec_rows(const nw_plan* p) { return with_geometry(p, p->uniq.U ? p->uniq.desc : p->desc); }

// One device chunk: (c, F, n) outputs of kind out_kind into dst (device); d = exec_rows(p).
int run_chunk(nw_plan* p, const nw::WDesc& d, const void* xs_dev, int64_t c, void* dst, int out_kind,
              bool dst_is_final) {
    if (!p->uniq.U) return run_chunk_rows(p, d, xs_dev, c, dst, out_kind, dst_is_final);
    const bool psum = out_kind == OUT_PSUM || out_kind == OUT_PHSUM;   // fp64 partial rows, one per block of signals
    const size_t row = psum ? (size_t)p->n_out() * sizeof(double) * (out_kind == OUT_PHSUM ? 2 : 1)
                            : (size_t)p->n_out() * (out_kind == NW_OUT_CWT ? 2 : 1) * p->esz;
    const int64_t crows = psum && !p->psum_per_signal ? nw::fused_psum_groups(c) : c;
    NW_TRY(p->d_uout.ensure((size_t)c * p->uniq.U * row));   // crows <= c
    // d_uout is scratch of the CWT's row size: K1 may write it
    NW_TRY(run_chunk_rows(p, d, xs_dev, c, p->d_uout.ptr, out_kind, true));
    // run_chunk_rows ends with a stage: chain onto it
    return NW_KERNEL_STAGE(p, ST_EXPAND, true,
                           nw::launch_expand_rows(p->d_uout.ptr, dst, crows, p->uniq.U, p->nfreq, row, p->uniq.offs,
                                                  p->uniq.order, p->stream));
}

bool is_reduction(int out_kind) { return out_kind >= NW_OUT_POWER_MEAN && out_kind <= NW_OUT_PHASE_SUM; }
bool is_phase(int out_kind) { return out_kind == NW_OUT_ITC || out_kind == NW_OUT_PHASE_SUM; }
// the out_kinds of nw_execute and the nw_execute_multi* calls
bool is_execute_kind(int out_kind) { return out_kind >= NW_OUT_CWT && out_kind <= NW_OUT_PHASE_SUM; }

// Host buffers: the chunk's `bytes` of input at xs staged into d_x, one copy stage
int stage_chunk(nw_plan* p, const void* xs, size_t bytes) {
    return staged(p, ST_COPY, [&] {
        NW_HIP(hipMemcpyAsync(p->d_x.ptr, xs, bytes, hipMemcpyHostToDevice, p->stream));
        return NW_OK;
    });
}

// The scratch a reduction's chunks leave their rows in: the rocFFT engine's run_chunk leaves y in d_Y;
// the other forms write d_out, grown to the caller's `bytes`
int reduce_scratch(nw_plan* p, size_t bytes, void** scratch) {
    if (p->form == FORM_ROCFFT) {
        NW_TRY(need_Y(p, p->nfreq));
        *scratch = p->d_Y.ptr;
    } else {
        NW_TRY(p->d_out.ensure(bytes));
        *scratch = p->d_out.ptr;
    }
    return NW_OK;
}

// The end of a reduction call: counted; with host buffers the result has landed and the stages are timed
int end_reduce(nw_plan* p, bool host) {
    p->stats.executes++;
    if (host) {
        NW_HIP(hipStreamSynchronize(p->stream));
        NW_TRY(resolve_timing(p));
    }
    return NW_OK;
}

// Epoch reductions (mneutils.py:42-71): every chunk's per-signal results (|y|^2 from
// the fused kernel, or y from the rocFFT engine's Y / the fused CWT for phases) are
// added in signal order into the fp64 accumulator; the (S, F, n) result never exists
// beyond one chunk.  nsig = 0 leaves acc = 0, so the mean is 0/0 = NaN like
// np.mean over an empty axis.
int execute_reduce(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nsig, void* out, int out_kind, bool host) {
    const bool phase = is_phase(out_kind);
    const int64_t fn = (int64_t)p->nfreq * p->n_out();
    const int64_t nacc = phase ? 2 * fn : fn;   // fp64 values of the accumulator (phase sums as 2 fn reals)
    const size_t acc_bytes = (size_t)nacc * sizeof(double);
    const bool fused = p->form != FORM_ROCFFT;
    // One-pass reductions with analytic rows: the kernel sums |y|^2 (ITC: y / |y|) over each block
    // of 8 signals in fp64, the accumulator adds the ceil(c / 8) fp64 partials (the same fp64
    // additions of the same values, grouped by 8 signals; with the dedup view
    // the partials of the distinct rows are expanded like any output row)
    // The chirp-z form (lengths 2n - 1 <= M_max, every row on chip) read-modify-writes its
    // block partial rows instead (no accumulator registers; any kind, fp32 and fp64); its
    // tentative lengths (rows may leave the chip) and the repeated-row view keep the chunk path;
    // so do complex table rows (MexicanHat, Haar, user tables), as on the fused form: their
    // partial-sum instantiations are not scratch-free (fp32 M = 4096: 20 B)
    bool chirp_psum = p->form == FORM_CHIRP && !p->chirp_tentative && !p->uniq.U && d.kind != NW_TABLE;
    if (chirp_psum) {
        NW_TRY(chirp_table(p, d));   // the rows' M classes decide (chirp_psum_ok)
        chirp_psum = !p->over.U && nw::chirp_psum_ok(p->dtype, phase, p->chirp_counts);
    }
    // (a decimated plan has no partial-sum kernel: its per-signal rows take the chunk path)
    const bool psum = (p->form == FORM_ONE_PASS && p->decim == 1 && nw::fused_psum_supported(p->n, p->dtype, d.kind, phase)) ||
                      chirp_psum;
    const int sig_kind = psum ? (phase ? OUT_PHSUM : OUT_PSUM) : (fused && !phase) ? NW_OUT_POWER : NW_OUT_CWT;
    // One-pass partial sums of a plan whose chunks are shorter than a signal group: the kernel's
    // accumulators are registers that start at zero, so a chunk cannot carry a group's row on as the
    // chirp-z kernel does.  Such a chunk leaves one fp64 row per signal (the terms a block adds),
    // which are added in signal order into the group's row `grp` behind the accumulator, and that
    // row is added to the accumulator once the group is complete: a block's additions, in its order.
    const bool per_signal = psum && !chirp_psum && p->max_batch < nw::kPsumGroup && nsig > p->max_batch;
    NW_TRY(p->d_acc.ensure(per_signal ? 2 * acc_bytes : acc_bytes));
    double* const acc = (double*)p->d_acc.ptr;
    double* const grp = acc + nacc;
    NW_HIP(hipMemsetAsync(acc, 0, per_signal ? 2 * acc_bytes : acc_bytes, p->stream));
    nw_logf(1, "plan %p: %s over %lld signals: %s", (void*)p, out_name(out_kind), (long long)nsig,
            psum ? "fp64 block partial sums inside the transform kernel"
                 : "per-signal rows per chunk, added in signal order in fp64");
    p->stats.reduce_path = psum ? NW_REDUCE_PARTIALS : NW_REDUCE_ROWS;
    // partials: plain fp64 sums (phase partials as 2 fn reals)
    const int src_kind = psum ? nw::ACC_POWER_REAL
                              : phase ? nw::ACC_PHASE_Y : (fused ? nw::ACC_POWER_REAL : nw::ACC_POWER_Y);
    size_t sb = (size_t)p->max_batch * fn * (phase ? 2 : 1) * p->esz;
    if (psum) sb = std::max(sb, (size_t)(per_signal ? p->max_batch : nw::fused_psum_groups(p->max_batch)) * acc_bytes);
    void* scratch = nullptr;
    NW_TRY(reduce_scratch(p, sb, &scratch));
    // The partial rows are those of the call's signal groups 0-7, 8-15, ... whatever max_batch
    // (chirp_psum_chunk), so the sums do not depend on it: a chirp-z chunk shorter than a group
    // carries the group's row on, and the row is added once the group is complete.
    for (int64_t s0 = 0, c = 0; s0 < nsig; s0 += c) {
        c = psum ? nw::chirp_psum_chunk(s0, nsig, p->max_batch) : std::min<int64_t>(p->max_batch, nsig - s0);
        const void* xs = (const char*)x + (size_t)s0 * p->n * p->esz;
        if (host) {
            NW_TRY(stage_chunk(p, xs, (size_t)c * p->n * p->esz));
            xs = p->d_x.ptr;
        }
        p->chirp_carry = chirp_psum && s0 % nw::kPsumGroup != 0;
        p->psum_per_signal = per_signal;
        const int rc = run_chunk(p, d, xs, c, scratch, sig_kind, false);
        p->chirp_carry = p->psum_per_signal = false;
        NW_TRY(rc);
        p->stats.chunks++;
        const bool goes_on = (s0 + c) % nw::kPsumGroup != 0 && s0 + c < nsig;   // the group: its next chunk follows
        // chained: run_chunk ends with a stage
        if (per_signal)
            NW_TRY(NW_KERNEL_STAGE(p, ST_EPI, true,
                                   nw::launch_accumulate(NW_F64, src_kind, scratch, grp, nacc, c, p->stream)));
        if ((chirp_psum || per_signal) && goes_on) continue;
        const int64_t rows = per_signal ? 1 : psum ? nw::fused_psum_groups(c) : c;
        NW_TRY(NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_accumulate(psum ? NW_F64 : p->dtype, src_kind, per_signal ? grp : scratch, acc,
                                                     psum ? nacc : fn, rows, p->stream)));
        if (per_signal) NW_HIP(hipMemsetAsync(grp, 0, acc_bytes, p->stream));
    }
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (out_kind == NW_OUT_POWER_SUM || out_kind == NW_OUT_PHASE_SUM) {
        NW_HIP(hipMemcpyAsync(out, acc, acc_bytes, back, p->stream));
    } else {
        // scratch is >= fn elements of the plan dtype on both engines
        void* dst = host ? scratch : out;
        NW_TRY(NW_KERNEL_STAGE(p, ST_EPI, false, nw::launch_finalize(p->dtype, phase, acc, dst, fn, nsig, p->stream)));
        if (host) NW_HIP(hipMemcpyAsync(out, dst, (size_t)fn * p->esz, hipMemcpyDeviceToHost, p->stream));
    }
    return end_reduce(p, host);
}

// Cross-channel pair reductions (nw_execute_pair): per chunk of max_batch / 2 pairs the two
// inputs are staged interleaved (a0, b0, a1, b1, ...) into d_x, the complex rows of the 2c
// signals go to the scratch execute_reduce uses (any form: the rows are n_out long), and
// k_accumulate_pair adds the pairs' products in pair order into the fp64 accumulator; where the
// signal-pair kernel forms them itself (pair_partials_supported) the chunk writes fp64 block
// partials instead and k_accumulate adds those.  The sums are returned as they are (npairs = 0:
// zeros).
int execute_pair(nw_plan* p, const nw::WDesc& d, const void* xa, const void* xb, int64_t npairs, void* out,
                 int out_kind, bool host) {
    const bool plv = out_kind == NW_OUT_PLV_SUM;
    const int mode = nw::sum_mode(out_kind);   // NW_OUT_LAG_SUM: four sums per point, always from the rows
    const int64_t fn = (int64_t)p->nfreq * p->n_out();
    const size_t acc_bytes = (size_t)fn * (plv ? 2 : 4) * sizeof(double);
    NW_TRY(p->d_acc.ensure(acc_bytes));
    double* const acc = (double*)p->d_acc.ptr;
    NW_HIP(hipMemsetAsync(acc, 0, acc_bytes, p->stream));
    // fp32 at the signal-pair kernel's sizes: the kernel sums each block's 4 pairs in fp64 and the
    // accumulator adds the ceil(2c / 8) partial rows (the same terms, regrouped); the decimated
    // form and the repeated-row view keep the chunk path.  NW_NO_PAIR_PARTIALS (diagnostics: the
    // A/B of tools/pair_rate.py) keeps it everywhere.
    const bool psum = p->form == FORM_ONE_PASS && p->decim == 1 && !p->uniq.U &&
                      nw::pair_partials_supported(p->n, p->dtype, d.kind, out_kind) && !std::getenv("NW_NO_PAIR_PARTIALS");
    const int comps = plv ? 2 : 4;
    nw_logf(1, "plan %p: %s over %lld pairs (%lld per chunk): %s", (void*)p, out_name(out_kind), (long long)npairs,
            (long long)(p->max_batch / 2),
            psum ? "fp64 block partial sums inside the transform kernel"
                 : "per-signal rows per chunk, added in pair order in fp64");
    p->stats.reduce_path = psum ? NW_REDUCE_PARTIALS : NW_REDUCE_ROWS;
    void* scratch = nullptr;
    NW_TRY(reduce_scratch(p, psum ? (size_t)nw::fused_psum_groups(p->max_batch) * fn * comps * sizeof(double)
                                  : (size_t)p->max_batch * fn * 2 * p->esz, &scratch));
    const int64_t per = p->max_batch / 2;
    const size_t row = (size_t)p->n * p->esz;
    const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    for (int64_t s0 = 0; s0 < npairs; s0 += per) {
        const int64_t c = std::min<int64_t>(per, npairs - s0);
        NW_TRY(staged(p, ST_COPY, [&] {
            // rows of `row` bytes, c of them, to every second row of d_x
            NW_HIP(hipMemcpy2DAsync(p->d_x.at(0), 2 * row, (const char*)xa + (size_t)s0 * row, row, row, (size_t)c, in,
                                    p->stream));
            NW_HIP(hipMemcpy2DAsync(p->d_x.at(row), 2 * row, (const char*)xb + (size_t)s0 * row, row, row, (size_t)c, in,
                                    p->stream));
            return NW_OK;
        }));
        NW_TRY(run_chunk(p, d, p->d_x.ptr, 2 * c, scratch, psum ? (plv ? OUT_PLVSUM : OUT_XSUM) : NW_OUT_CWT, false));
        // chained: run_chunk ends with a stage
        if (psum)   // partials: plain fp64 sums over comps * fn values
            NW_TRY(NW_KERNEL_STAGE(p, ST_EPI, true,
                                   nw::launch_accumulate(NW_F64, nw::ACC_POWER_REAL, scratch, acc, comps * fn,
                                                         nw::fused_psum_groups(2 * c), p->stream)));
        else
            NW_TRY(NW_KERNEL_STAGE(p, ST_EPI, true,
                                   nw::launch_accumulate_pair(p->dtype, mode, scratch, acc, fn, c, p->stream)));
        p->stats.chunks++;
    }
    NW_HIP(hipMemcpyAsync(out, acc, acc_bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, p->stream));
    return end_reduce(p, host);
}

// The epoch-chunk reductions (nw_execute_conn, _conn_time, _env_time, _pac, _pac_surr, _pac_bins, _erpac) share one layout of d_acc
// and one loop.  d_acc holds the call's fp64 output regions one after the other and then, 16-aligned,
// one auxiliary blob (tile descriptors or index lists) that is built and uploaded once per call.
struct SumRegion {
    void* out;            // the caller's buffer
    size_t bytes;         // of the whole call; an optional output that was not asked for has out = null, bytes = 0
    size_t epoch;         // of one epoch (0: the region belongs to the call as a whole and is read-modify-written)
    char* dev = nullptr;  // its place in d_acc (the first region always has one; a later one without `out`: null)
    char* at(int64_t e0) const { return dev ? dev + (size_t)e0 * epoch : nullptr; }
};

// Places the regions and the blob and uploads the blob; zero: the regions start at 0 (sums that are
// read-modify-written per chunk).  `what` completes the message of a failed allocation.
int place_sums(nw_plan* p, SumRegion* r, int nr, const void* aux, size_t aux_bytes, const char** d_aux, bool zero,
               const std::string& what) {
    size_t acc_bytes = 0;
    for (int i = 0; i < nr; ++i) acc_bytes += r[i].bytes;   // multiples of 8
    const size_t aux_at = (acc_bytes + 15) / 16 * 16;
    const int got = p->d_acc.ensure(aux_at + aux_bytes + 16);
    if (got != NW_OK && got != NW_E_NOMEM) return got;
    if (got == NW_E_NOMEM)
        return fail(NW_E_NOMEM, what + " need " + std::to_string(aux_at + aux_bytes + 16) +
                                    " bytes of device memory: " + g_last_error);
    size_t at = 0;
    for (int i = 0; i < nr; ++i) {
        r[i].dev = i == 0 || r[i].out ? p->d_acc.at(at) : nullptr;
        at += r[i].bytes;
    }
    *d_aux = p->d_acc.at(aux_at);
    if (zero && acc_bytes) NW_HIP(hipMemsetAsync(p->d_acc.at(0), 0, acc_bytes, p->stream));
    if (aux_bytes) NW_HIP(hipMemcpyAsync((void*)*d_aux, aux, aux_bytes, hipMemcpyHostToDevice, p->stream));
    return NW_OK;
}

// block order: the blocks that share rows neighbours on one XCD (conn_slot, conn_time_slot, pac_slot);
// NW_CONN_PLAIN_ORDER (diagnostics: the A/B of tools/conn_rate.py) keeps plain block order
bool xcd_order() { return !std::getenv("NW_CONN_PLAIN_ORDER"); }

// Per chunk of max_batch / nchan epochs the (ec, nchan, n) block of x is staged as it lies
// (epoch-major), the complex rows of its ec * nchan signals go to the scratch execute_pair uses (any
// form), and launch(e0, ec, rows) reduces them -- one kernel stage, chained: run_chunk ends with a
// stage.  Then the regions are copied to the caller's buffers, once.
template <typename F>
int run_epoch_chunks(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const SumRegion* r,
                     int nr, bool host, F&& launch) {
    void* scratch = nullptr;
    NW_TRY(reduce_scratch(p, (size_t)p->max_batch * p->nfreq * p->n_out() * 2 * p->esz, &scratch));
    const int64_t per = p->max_batch / nchan;
    const size_t epoch_bytes = (size_t)nchan * p->n * p->esz;
    for (int64_t e0 = 0; e0 < nepochs; e0 += per) {
        const int64_t ec = std::min<int64_t>(per, nepochs - e0);
        const void* xs = (const char*)x + (size_t)e0 * epoch_bytes;
        if (host) {
            NW_TRY(stage_chunk(p, xs, (size_t)ec * epoch_bytes));
            xs = p->d_x.ptr;
        }
        NW_TRY(run_chunk(p, d, xs, ec * nchan, scratch, NW_OUT_CWT, false));
        NW_TRY(launch(e0, ec, scratch));
        p->stats.chunks++;
    }
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    for (int i = 0; i < nr; ++i)
        if (r[i].bytes) NW_HIP(hipMemcpyAsync(r[i].out, r[i].dev, r[i].bytes, back, p->stream));
    return end_reduce(p, host);
}

// Multi-channel connectivity (nw_execute_conn): per chunk nw_conn_accumulate_kernel adds every pair's
// products of the chunk into the fp64 accumulators, which it reads and writes once per chunk;
// nw_conn_power_kernel adds |y|^2 per channel.
int execute_conn(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ia,
                 const int32_t* ib, int64_t npairs, void* out_cross, void* out_power, int out_kind, bool host) {
    const int mode = nw::sum_mode(out_kind);
    const int64_t fn = (int64_t)p->nfreq * p->n_out();
    // 16 B per pair and point (a complex fp64), NW_OUT_LAG_SUM: 32 B (its four sums)
    SumRegion r[2] = {{out_cross, (size_t)npairs * fn * (mode == nw::SUM_LAG ? 4 : 2) * sizeof(double), 0},
                      {out_power, out_power ? (size_t)nchan * fn * sizeof(double) : 0, 0}};
    p->conn_tiles = nw::host::conn_tiles(ia, ib, npairs, nullptr);
    const int ntiles = (int)p->conn_tiles.size();
    const char* tiles = nullptr;
    NW_TRY(place_sums(p, r, 2, p->conn_tiles.data(), ntiles * sizeof(nw::ConnTile), &tiles, true,
                      "nw_execute_conn: the fp64 accumulators of " + std::to_string(npairs) + " pairs and " +
                          std::to_string(out_power ? nchan : 0) + " channels"));
    const bool xcd = xcd_order();
    nw_logf(1, "plan %p: %s over %lld epochs x %d channels, %lld pairs in %lld tiles (%lld epochs per chunk): "
               "per-signal rows per chunk, every pair added in epoch order in fp64",
            (void*)p, out_name(out_kind), (long long)nepochs, nchan, (long long)npairs, (long long)ntiles,
            (long long)(p->max_batch / nchan));
    p->stats.reduce_path = NW_REDUCE_CONN;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 2, host, [&](int64_t, int64_t ec, void* rows) {
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_conn_accumulate(p->dtype, mode, rows, r[0].dev, (double*)r[1].dev,
                                                          (const nw::ConnTile*)tiles, ntiles, ec, nchan, p->nfreq,
                                                          p->n_out(), npairs, xcd, p->stream));
    });
}

// the log line of the over-time pair sums (after place_time_sums: it counts the call's tiles)
void log_time_sums(nw_plan* p, const char* name, int64_t nepochs, int nchan, int64_t npairs, int64_t t0, int64_t t1,
                   int64_t step, bool host) {
    nw_logf(1, "plan %p: %s over time, %lld epochs x %d channels, %lld pairs in %lld tiles (%lld epochs per chunk), "
               "window [%lld, %lld) step %lld of %lld samples, %s buffers: per-signal rows per chunk, every (epoch, "
               "pair, scale) summed over its %lld samples in fp64 in lane order",
            (void*)p, name, (long long)nepochs, nchan, (long long)npairs, (long long)p->conn_tiles.size(),
            (long long)(p->max_batch / nchan), (long long)t0, (long long)t1, (long long)step, (long long)p->n_out(),
            host ? "host" : "device", (long long)nw::conn_time_count(t0, t1, step));
}

// The regions of the over-time pair sums: pair_vals fp64 per (e, p, f) and, where out_chan is given,
// chan_vals per (e, c, f); the blob is the call's tile descriptors (p->conn_tiles).
int place_time_sums(nw_plan* p, const char* who, SumRegion (&r)[2], int64_t nepochs, int nchan, const int32_t* ia,
                    const int32_t* ib, int64_t npairs, void* out_pair, int pair_vals, void* out_chan, int chan_vals,
                    const nw::ConnTile** tiles) {
    const size_t pair_epoch = (size_t)npairs * p->nfreq * pair_vals * sizeof(double);
    const size_t chan_epoch = (size_t)nchan * p->nfreq * chan_vals * sizeof(double);
    r[0] = {out_pair, (size_t)nepochs * pair_epoch, pair_epoch};
    r[1] = {out_chan, out_chan ? (size_t)nepochs * chan_epoch : 0, chan_epoch};
    p->conn_tiles = nw::host::conn_tiles(ia, ib, npairs, nullptr);
    return place_sums(p, r, 2, p->conn_tiles.data(), p->conn_tiles.size() * sizeof(nw::ConnTile), (const char**)tiles, false,
                      std::string(who) + ": the fp64 sums of " + std::to_string(nepochs) + " epochs, " +
                          std::to_string(npairs) + " pairs and " + std::to_string(out_chan ? nchan : 0) + " channels");
}

// Over-time connectivity (nw_execute_conn_time): per chunk nw_conn_time_kernel reduces every pair's
// products along the window's `count` samples t0 + j * step and writes the chunk's epochs' slice of the
// (E, P, F) sums, nw_conn_time_power_kernel the (E, C, F) power sums.  Every value is written by exactly
// one block of one launch: no memset.
int execute_conn_time(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ia,
                      const int32_t* ib, int64_t npairs, int64_t t0, int64_t t1, int64_t step, void* out_sum,
                      void* out_power, int out_kind, bool host) {
    const int mode = nw::sum_mode(out_kind);
    const int64_t count = nw::conn_time_count(t0, t1, step);
    SumRegion r[2];
    const nw::ConnTile* tiles = nullptr;
    NW_TRY(place_time_sums(p, "nw_execute_conn_time", r, nepochs, nchan, ia, ib, npairs, out_sum,
                           mode == nw::SUM_LAG ? 4 : 2, out_power, 1, &tiles));
    const bool xcd = xcd_order();
    log_time_sums(p, out_name(out_kind), nepochs, nchan, npairs, t0, t1, step, host);
    p->stats.reduce_path = NW_REDUCE_CONN_TIME;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 2, host, [&](int64_t e0, int64_t ec, void* rows) -> int {
        if (npairs == 0 && !r[1].dev) return NW_OK;
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_conn_time(p->dtype, mode, rows, r[0].at(e0), (double*)r[1].at(e0), tiles,
                                                    (int)p->conn_tiles.size(), ec, nchan, p->nfreq, p->n_out(), npairs,
                                                    t0, count, step, xcd, p->stream));
    });
}

// Envelope correlation (nw_execute_env_time): as execute_conn_time with nw_env_time_kernel's pair sums
// (1 or 6 fp64 per (e, p, f)) and nw_env_chan_kernel's per-channel sums (2 fp64 per (e, c, f)).
int execute_env_time(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ia,
                     const int32_t* ib, int64_t npairs, int64_t t0, int64_t t1, int64_t step, void* out_pair,
                     void* out_chan, int env, bool host) {
    const int64_t count = nw::conn_time_count(t0, t1, step);
    SumRegion r[2];
    const nw::ConnTile* tiles = nullptr;
    NW_TRY(place_time_sums(p, "nw_execute_env_time", r, nepochs, nchan, ia, ib, npairs, out_pair,
                           nw::env_pair_values(env), out_chan, 2, &tiles));
    const bool xcd = xcd_order();
    log_time_sums(p, env == NW_ENV_ORTH ? "env_orth_sum" : "env_sum", nepochs, nchan, npairs, t0, t1, step, host);
    p->stats.reduce_path = NW_REDUCE_ENV;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 2, host, [&](int64_t e0, int64_t ec, void* rows) -> int {
        if (npairs == 0 && !r[1].dev) return NW_OK;
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_env_time(p->dtype, env, rows, r[0].at(e0), (double*)r[1].at(e0), tiles,
                                                   (int)p->conn_tiles.size(), ec, nchan, p->nfreq, p->n_out(), npairs,
                                                   t0, count, step, xcd, p->stream));
    });
}

// Phase-amplitude coupling (nw_execute_pac): per chunk nw_pac_kernel reduces every pair's |y_a| u_p
// products along the window's `count` samples for every listed (phase, amplitude) scale and writes the
// chunk's epochs' slice of the (E, P, nph, nam) sums, nw_pac_rows_kernel the per-channel sums.  The blob is
// the pair and scale lists.  Every value is written by exactly one block of one launch: no memset.
int execute_pac(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ip,
                const int32_t* ia, int64_t npairs, const int32_t* fph, int nph, const int32_t* fam, int nam,
                int64_t t0, int64_t t1, int64_t step, void* out_m, void* out_amp, void* out_phase, bool host) {
    const int64_t count = nw::conn_time_count(t0, t1, step);
    const size_t m_epoch = (size_t)npairs * nph * nam * 2 * sizeof(double);        // of one epoch
    const size_t amp_epoch = (size_t)nchan * nam * 2 * sizeof(double);
    const size_t phase_epoch = (size_t)nchan * nph * 2 * sizeof(double);
    SumRegion r[3] = {{out_m, (size_t)nepochs * m_epoch, m_epoch},
                      {out_amp, out_amp ? (size_t)nepochs * amp_epoch : 0, amp_epoch},
                      {out_phase, out_phase ? (size_t)nepochs * phase_epoch : 0, phase_epoch}};
    std::vector<int32_t>& lists = p->pac_lists;                   // ip, ia, fph, fam
    lists.clear();
    lists.insert(lists.end(), ip, ip + npairs);
    lists.insert(lists.end(), ia, ia + npairs);
    lists.insert(lists.end(), fph, fph + nph);
    lists.insert(lists.end(), fam, fam + nam);
    const char* d_lists = nullptr;
    NW_TRY(place_sums(p, r, 3, lists.data(), lists.size() * sizeof(int32_t), &d_lists, false,
                      "nw_execute_pac: the fp64 sums of " + std::to_string(nepochs) + " epochs, " + std::to_string(npairs) +
                          " pairs and " + std::to_string(nph) + " x " + std::to_string(nam) + " scales"));
    const int32_t* const d_ip = (const int32_t*)d_lists;
    const int32_t* const d_ia = d_ip + npairs;
    const int32_t* const d_fph = d_ia + npairs;
    const int32_t* const d_fam = d_fph + nph;
    const bool xcd = xcd_order();
    nw_logf(1, "plan %p: pac sums, %lld epochs x %d channels, %lld pairs, %d phase x %d amplitude scales in %lld tiles "
               "(%lld epochs per chunk), window [%lld, %lld) step %lld of %lld samples, %s buffers: per-signal rows per "
               "chunk, every (epoch, pair, phase scale, amplitude scale) summed over its %lld samples in fp64 in lane "
               "order",
            (void*)p, (long long)nepochs, nchan, (long long)npairs, nph, nam, (long long)nw::pac_tiles(nph, nam),
            (long long)(p->max_batch / nchan), (long long)t0, (long long)t1, (long long)step, (long long)p->n_out(),
            host ? "host" : "device", (long long)count);
    p->stats.reduce_path = NW_REDUCE_PAC;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 3, host, [&](int64_t e0, int64_t ec, void* rows) -> int {
        if (!(r[0].bytes + r[1].bytes + r[2].bytes)) return NW_OK;
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_pac(p->dtype, rows, r[0].at(e0), r[1].at(e0), r[2].at(e0), d_ip, d_ia, d_fph,
                                              d_fam, ec, nchan, p->nfreq, p->n_out(), npairs, nph, nam, t0, count, step,
                                              xcd, p->stream));
    });
}

// Time-lag surrogates of the coupling (nw_execute_pac_surr): execute_pac's regions, then the statistics and, where
// asked, every surrogate sum; the blob is the pair and scale lists, padded to 16 bytes, and then the lags.  Per
// chunk, one kernel stage: nw_pac_rows_kernel's per-channel sums (into the caller's regions, or into the tail of
// d_pstage: the debiased centring reads them), nw_pac_stage_kernel's unit phasors and magnitudes of the chunk into
// d_pstage, and nw_pac_surr_kernel, which writes the chunk's epochs' slice of M, the statistics and the surrogates.
int execute_pac_surr(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ip,
                     const int32_t* ia, int64_t npairs, const int32_t* fph, int nph, const int32_t* fam, int nam,
                     int64_t t0, int64_t t1, int64_t step, const int64_t* lags, int nlags, int centre, void* out_m,
                     void* out_amp, void* out_phase, void* out_stat, void* out_all, bool host) {
    const int64_t count = nw::conn_time_count(t0, t1, step);
    const size_t cells = (size_t)npairs * nph * nam;                               // of one epoch
    const size_t amp_epoch = (size_t)nchan * nam * 2 * sizeof(double);
    const size_t phase_epoch = (size_t)nchan * nph * 2 * sizeof(double);
    const size_t stat_epoch = cells * 4 * sizeof(double), all_epoch = cells * nlags * 2 * sizeof(double);
    SumRegion r[5] = {{out_m, (size_t)nepochs * cells * 2 * sizeof(double), cells * 2 * sizeof(double)},
                      {out_amp, out_amp ? (size_t)nepochs * amp_epoch : 0, amp_epoch},
                      {out_phase, out_phase ? (size_t)nepochs * phase_epoch : 0, phase_epoch},
                      {out_stat, out_stat ? (size_t)nepochs * stat_epoch : 0, stat_epoch},
                      {out_all, out_all ? (size_t)nepochs * all_epoch : 0, all_epoch}};
    std::vector<int32_t>& lists = p->pac_lists;                   // ip, ia, fph, fam, padding, the lags
    lists.clear();
    lists.insert(lists.end(), ip, ip + npairs);
    lists.insert(lists.end(), ia, ia + npairs);
    lists.insert(lists.end(), fph, fph + nph);
    lists.insert(lists.end(), fam, fam + nam);
    lists.resize((lists.size() + 3) / 4 * 4, 0);
    const size_t lags_at = lists.size();
    lists.resize(lags_at + (size_t)nlags * 2);
    if (nlags) std::memcpy(lists.data() + lags_at, lags, (size_t)nlags * sizeof(int64_t));
    const std::string what = "nw_execute_pac_surr: the fp64 sums of " + std::to_string(nepochs) + " epochs, " +
                             std::to_string(npairs) + " pairs, " + std::to_string(nph) + " x " + std::to_string(nam) +
                             " scales and " + std::to_string(nlags) + " lags";
    const char* d_lists = nullptr;
    NW_TRY(place_sums(p, r, 5, lists.data(), lists.size() * sizeof(int32_t), &d_lists, false, what));
    // one chunk's staged values and, after them, its per-channel sums
    const int64_t per = std::min<int64_t>(p->max_batch / nchan, std::max<int64_t>(nepochs, 1));
    const size_t stage_bytes = (size_t)nw::pac_surr_stage_doubles(per * nchan, nph, nam, count) * sizeof(double);
    const int got = p->d_pstage.ensure(stage_bytes + (size_t)per * (amp_epoch + phase_epoch) + 16);
    if (got != NW_OK && got != NW_E_NOMEM) return got;
    if (got == NW_E_NOMEM)
        return fail(NW_E_NOMEM, what + ": the staged unit phasors and magnitudes of a chunk of " + std::to_string(per) +
                                    " epochs need " + std::to_string(stage_bytes) + " bytes of device memory: " + g_last_error);
    char* const spare_amp = p->d_pstage.at(stage_bytes);
    char* const spare_phase = spare_amp + (size_t)per * amp_epoch;
    const int32_t* const d_ip = (const int32_t*)d_lists;
    const int32_t* const d_ia = d_ip + npairs;
    const int32_t* const d_fph = d_ia + npairs;
    const int32_t* const d_fam = d_fph + nph;
    const int64_t* const d_lags = (const int64_t*)((const int32_t*)d_lists + lags_at);
    const bool xcd = xcd_order();
    nw_logf(1, "plan %p: pac surrogate sums (%s), %lld epochs x %d channels, %lld pairs, %d phase x %d amplitude scales "
               "in %lld tiles, %d lags%s (%lld epochs per chunk, %lld B staged), window [%lld, %lld) step %lld of %lld "
               "samples, %s buffers: per-signal rows per chunk, staged once as unit phasors and magnitudes, every "
               "(epoch, pair, phase scale, amplitude scale) summed over its %lld samples once per lag in fp64 in lane order",
            (void*)p, centre == NW_PAC_SURR_DEBIASED ? "debiased" : "plain", (long long)nepochs, nchan,
            (long long)npairs, nph, nam, (long long)nw::pac_tiles(nph, nam), nlags, out_all ? ", every sum kept" : "",
            (long long)(p->max_batch / nchan), (long long)stage_bytes, (long long)t0, (long long)t1, (long long)step,
            (long long)p->n_out(), host ? "host" : "device", (long long)count);
    p->stats.reduce_path = NW_REDUCE_PAC_SURR;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 5, host, [&](int64_t e0, int64_t ec, void* rows) -> int {
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_pac_surr(p->dtype, rows, p->d_pstage.ptr, r[0].at(e0),
                                                   r[1].dev ? r[1].at(e0) : spare_amp,
                                                   r[2].dev ? r[2].at(e0) : spare_phase, r[3].at(e0), r[4].at(e0), d_ip,
                                                   d_ia, d_fph, d_fam, d_lags, nlags, centre, ec, nchan, p->nfreq,
                                                   p->n_out(), npairs, nph, nam, t0, count, step, xcd, p->stream));
    });
}

// Event-related phase-amplitude coupling (nw_execute_erpac): execute_pac's staging and lists with the sums
// taken over the epochs: per chunk nw_erpac_kernel adds the chunk's epochs to the (P, nph, nam, T) sums, which
// it reads and writes once per chunk, and nw_erpac_rows_kernel to the per-channel sums.  The three regions
// belong to the call as a whole (epoch = 0) and start at zero.
int execute_erpac(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ip,
                  const int32_t* ia, int64_t npairs, const int32_t* fph, int nph, const int32_t* fam, int nam,
                  int64_t t0, int64_t t1, int64_t step, void* out_m, void* out_amp, void* out_phase, bool host) {
    const int64_t count = nw::conn_time_count(t0, t1, step);
    SumRegion r[3] = {{out_m, (size_t)npairs * nph * nam * count * 2 * sizeof(double), 0},
                      {out_amp, out_amp ? (size_t)nchan * nam * count * 2 * sizeof(double) : 0, 0},
                      {out_phase, out_phase ? (size_t)nchan * nph * count * 5 * sizeof(double) : 0, 0}};
    std::vector<int32_t>& lists = p->pac_lists;                   // ip, ia, fph, fam
    lists.clear();
    lists.insert(lists.end(), ip, ip + npairs);
    lists.insert(lists.end(), ia, ia + npairs);
    lists.insert(lists.end(), fph, fph + nph);
    lists.insert(lists.end(), fam, fam + nam);
    const char* d_lists = nullptr;
    NW_TRY(place_sums(p, r, 3, lists.data(), lists.size() * sizeof(int32_t), &d_lists, true,
                      "nw_execute_erpac: the fp64 accumulators of " + std::to_string(npairs) + " pairs, " +
                          std::to_string(nph) + " x " + std::to_string(nam) + " scales and " + std::to_string(count) +
                          " samples"));
    const int32_t* const d_ip = (const int32_t*)d_lists;
    const int32_t* const d_ia = d_ip + npairs;
    const int32_t* const d_fph = d_ia + npairs;
    const int32_t* const d_fam = d_fph + nph;
    const bool xcd = xcd_order();
    nw_logf(1, "plan %p: erpac sums, %lld epochs x %d channels, %lld pairs, %d phase x %d amplitude scales in %lld tiles "
               "x %lld sample tiles (%lld epochs per chunk), window [%lld, %lld) step %lld of %lld samples, %s buffers: "
               "per-signal rows per chunk, every (pair, phase scale, amplitude scale, sample) of the window's %lld added "
               "in epoch order in fp64",
            (void*)p, (long long)nepochs, nchan, (long long)npairs, nph, nam, (long long)nw::pac_tiles(nph, nam),
            (long long)nw::erpac_sample_tiles(count), (long long)(p->max_batch / nchan), (long long)t0, (long long)t1,
            (long long)step, (long long)p->n_out(), host ? "host" : "device", (long long)count);
    p->stats.reduce_path = NW_REDUCE_ERPAC;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 3, host, [&](int64_t, int64_t ec, void* rows) -> int {
        if (!(r[0].bytes + r[1].bytes + r[2].bytes)) return NW_OK;
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_erpac(p->dtype, rows, r[0].dev, r[1].dev, r[2].dev, d_ip, d_ia, d_fph, d_fam,
                                                ec, nchan, p->nfreq, p->n_out(), npairs, nph, nam, t0, count, step, xcd,
                                                p->stream));
    });
}

// the table of nw_pac_bin_edges: cs[b] = {cos theta_b, sin theta_b}, theta_b = -pi + 2 pi b / nbins
void pac_bin_edges(int nbins, double* cs) {
    const double pi = 3.14159265358979323846;
    for (int b = 0; b < nbins; ++b) {
        const double theta = -pi + 2.0 * pi * b / nbins;
        cs[2 * b] = std::cos(theta);
        cs[2 * b + 1] = std::sin(theta);
    }
}

// Phase-binned phase-amplitude coupling (nw_execute_pac_bins): as execute_pac with nw_pac_bins_kernel's
// (E, P, nph, nam, nbins) sums and nw_pac_bins_rows_kernel's (E, C, nph, nbins) counts.  The blob is the
// pair and scale lists, padded to 16 bytes, and then the edge table the kernels read.
int execute_pac_bins(nw_plan* p, const nw::WDesc& d, const void* x, int64_t nepochs, int nchan, const int32_t* ip,
                     const int32_t* ia, int64_t npairs, const int32_t* fph, int nph, const int32_t* fam, int nam,
                     int64_t t0, int64_t t1, int64_t step, int nbins, void* out_sum, void* out_count, bool host) {
    const int64_t count = nw::conn_time_count(t0, t1, step);
    const size_t sum_epoch = (size_t)npairs * nph * nam * nbins * sizeof(double);   // of one epoch
    const size_t count_epoch = (size_t)nchan * nph * nbins * sizeof(double);
    SumRegion r[2] = {{out_sum, (size_t)nepochs * sum_epoch, sum_epoch},
                      {out_count, out_count ? (size_t)nepochs * count_epoch : 0, count_epoch}};
    std::vector<int32_t>& lists = p->pac_lists;                   // ip, ia, fph, fam, padding, the edge table
    lists.clear();
    lists.insert(lists.end(), ip, ip + npairs);
    lists.insert(lists.end(), ia, ia + npairs);
    lists.insert(lists.end(), fph, fph + nph);
    lists.insert(lists.end(), fam, fam + nam);
    lists.resize((lists.size() + 3) / 4 * 4, 0);
    const size_t edges_at = lists.size();
    double cs[2 * NW_PAC_MAX_BINS];
    pac_bin_edges(nbins, cs);
    lists.resize(edges_at + (size_t)nbins * 4);
    std::memcpy(lists.data() + edges_at, cs, (size_t)nbins * 2 * sizeof(double));
    const char* d_lists = nullptr;
    NW_TRY(place_sums(p, r, 2, lists.data(), lists.size() * sizeof(int32_t), &d_lists, false,
                      "nw_execute_pac_bins: the fp64 sums of " + std::to_string(nepochs) + " epochs, " +
                          std::to_string(npairs) + " pairs and " + std::to_string(nph) + " x " + std::to_string(nam) +
                          " scales x " + std::to_string(nbins) + " bins"));
    const int32_t* const d_ip = (const int32_t*)d_lists;
    const int32_t* const d_ia = d_ip + npairs;
    const int32_t* const d_fph = d_ia + npairs;
    const int32_t* const d_fam = d_fph + nph;
    const void* const d_edges = (const int32_t*)d_lists + edges_at;
    const bool xcd = xcd_order();
    nw_logf(1, "plan %p: pac bin sums, %lld epochs x %d channels, %lld pairs, %d phase x %d amplitude scales x %d bins "
               "in %lld tiles of %d amplitude scales, %lld B of LDS per block (%lld epochs per chunk), window [%lld, "
               "%lld) step %lld of %lld samples, %s buffers: per-signal rows per chunk, every (epoch, pair, phase "
               "scale, amplitude scale, bin) summed over its samples of the window's %lld in fp64 in lane order",
            (void*)p, (long long)nepochs, nchan, (long long)npairs, nph, nam, nbins,
            (long long)nw::pac_bins_tiles(nph, nam, nbins), nw::pac_bins_am(nbins), (long long)nw::pac_bins_lds(nbins),
            (long long)(p->max_batch / nchan), (long long)t0, (long long)t1, (long long)step, (long long)p->n_out(),
            host ? "host" : "device", (long long)count);
    p->stats.reduce_path = NW_REDUCE_PAC_BINS;
    return run_epoch_chunks(p, d, x, nepochs, nchan, r, 2, host, [&](int64_t e0, int64_t ec, void* rows) -> int {
        if (!(r[0].bytes + r[1].bytes)) return NW_OK;
        return NW_KERNEL_STAGE(p, ST_EPI, true,
                               nw::launch_pac_bins(p->dtype, rows, r[0].at(e0), r[1].at(e0), d_ip, d_ia, d_fph, d_fam,
                                                   d_edges, ec, nchan, p->nfreq, p->n_out(), npairs, nph, nam, nbins, t0,
                                                   count, step, xcd, p->stream));
    });
}

// the scale lists of nw_execute_pac and nw_execute_pac_bins: positions inside the plan's scale list
int check_scale_lists(const char* who, const nw_plan* p, const int32_t* fph, int32_t nph, const int32_t* fam,
                      int32_t nam) {
    const std::string w = std::string(who) + ": ";
    if (nph < 0 || nam < 0) return fail(NW_E_INVALID, w + "nph < 0 or nam < 0");
    if ((nph > 0 && !fph) || (nam > 0 && !fam)) return fail(NW_E_INVALID, w + "null scale list");
    for (int which = 0; which < 2; ++which) {
        const int32_t* const f = which ? fam : fph;
        for (int32_t i = 0; i < (which ? nam : nph); ++i)
            if (f[i] < 0 || f[i] >= p->nfreq)
                return fail(NW_E_INVALID, w + (which ? "amplitude" : "phase") + " scale " + std::to_string(i) + " = " +
                                              std::to_string(f[i]) + " is outside [0, " + std::to_string(p->nfreq) + ")");
    }
    return NW_OK;
}

// nbins of nw_pac_bin_edges and nw_execute_pac_bins
int check_nbins(const char* who, int32_t nbins) {
    if (!nw::pac_bins_valid(nbins))
        return fail(NW_E_INVALID, std::string(who) + ": nbins (" + std::to_string(nbins) + ") must be even with 2 <= nbins <= " +
                                      std::to_string(NW_PAC_MAX_BINS));
    return NW_OK;
}

// the pair list of nw_conn_tiles / nw_execute_conn: indices inside [0, nchan)
int check_pairs(const char* who, int32_t nchan, const int32_t* ia, const int32_t* ib, int64_t npairs) {
    if (nchan < 1) return fail(NW_E_INVALID, std::string(who) + ": nchan < 1");
    if (npairs < 0) return fail(NW_E_INVALID, std::string(who) + ": npairs < 0");
    if (npairs > 0x7fffffff) return fail(NW_E_INVALID, std::string(who) + ": more than 2^31 - 1 pairs");
    if (npairs > 0 && (!ia || !ib)) return fail(NW_E_INVALID, std::string(who) + ": null pair list");
    for (int64_t q = 0; q < npairs; ++q)
        if (ia[q] < 0 || ia[q] >= nchan || ib[q] < 0 || ib[q] >= nchan)
            return fail(NW_E_INVALID, std::string(who) + ": pair " + std::to_string(q) + " = (" + std::to_string(ia[q]) +
                                          ", " + std::to_string(ib[q]) + ") is outside [0, " + std::to_string(nchan) + ")");
    return NW_OK;
}

// the checks the epoch-chunk calls share, in the order they always had; null_arg and kind_error (the
// call's complaint about its out_kind or env_kind, or null) are the caller's own findings
int check_epoch_call(const char* who, const nw_plan* p, bool null_arg, const char* kind_error, int mem, int64_t nepochs,
                     int32_t nchan, const int32_t* ia, const int32_t* ib, int64_t npairs) {
    const std::string w = std::string(who) + ": ";
    if (null_arg) return fail(NW_E_INVALID, w + "null argument");
    if (!p->has_wavelet) return fail(NW_E_STATE, w + "nw_plan_set_wavelet first");
    if (kind_error) return fail(NW_E_INVALID, w + kind_error);
    if (mem != NW_MEM_HOST && mem != NW_MEM_DEVICE) return fail(NW_E_INVALID, w + "bad mem");
    if (nepochs < 0) return fail(NW_E_INVALID, w + "nepochs < 0");
    return check_pairs(who, nchan, ia, ib, npairs);
}

// a chunk holds whole epochs
int check_chunk(const char* who, const nw_plan* p, int32_t nchan) {
    if (p->max_batch < nchan)
        return fail(NW_E_INVALID, std::string(who) + ": the plan's max_batch (" + std::to_string(p->max_batch) +
                                      ") must be >= nchan (" + std::to_string(nchan) +
                                      "): a chunk holds max_batch / nchan epochs");
    return NW_OK;
}

// the window [t0, t1) and its step of the over-time sums
int check_window(const char* who, int64_t n_out, int64_t t0, int64_t t1, int64_t step) {
    if (step < 1) return fail(NW_E_INVALID, std::string(who) + ": step (" + std::to_string(step) + ") must be >= 1");
    if (t0 < 0 || t0 > t1 || t1 > n_out)
        return fail(NW_E_INVALID, std::string(who) + ": the window [" + std::to_string(t0) + ", " + std::to_string(t1) +
                                      ") must satisfy 0 <= t0 <= t1 <= n_out (" + std::to_string(n_out) + ")");
    return NW_OK;
}

// the out_kind of nw_execute_pair (no out_power), nw_execute_conn and nw_execute_conn_time: null, or
// what is wrong with it
const char* conn_kind_error(int out_kind, const void* out_power) {
    if (out_kind != NW_OUT_CROSS_SUM && out_kind != NW_OUT_PLV_SUM && out_kind != NW_OUT_LAG_SUM)
        return "out_kind must be NW_OUT_CROSS_SUM, NW_OUT_PLV_SUM or NW_OUT_LAG_SUM";
    if (out_kind == NW_OUT_PLV_SUM && out_power) return "NW_OUT_PLV_SUM forms no power sums: out_power must be NULL";
    if (out_kind == NW_OUT_LAG_SUM && out_power) return "NW_OUT_LAG_SUM forms no power sums: out_power must be NULL";
    return nullptr;
}

// the start of an execute call (under the caller's DeviceGuard): the rows of this call
int begin_execute(nw_plan* p, nw::WDesc* d) {
    p->executed = true;
    *d = exec_rows(p);
    // settle the form of a tentative length before any buffer choice
    if (p->form == FORM_CHIRP && p->chirp_tentative) NW_TRY(chirp_table(p, *d));
    return NW_OK;
}

// ---- page-locked result buffers (nw_host_alloc): a destination inside one is written by DMA
std::mutex g_host_mu;
std::map<uintptr_t, size_t> g_host_bufs;   // base -> bytes

bool host_pinned(const void* p, size_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_bufs.upper_bound(a);
    if (it == g_host_bufs.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

// ---- host-buffer copy-out: pinned double-buffered pieces + a multi-threaded host copy
constexpr size_t kPiece = size_t(64) << 20;
// host copy threads (NW_COPY_THREADS overrides, diagnostics)
int copy_threads() {
    static const int n = [] {
        const char* e = std::getenv("NW_COPY_THREADS");
        const int v = e ? std::atoi(e) : 8;
        return v > 0 ? v : 8;
    }();
    return n;
}

int copy_out(nw_plan* p, char* dst, const char* src, size_t bytes) {
    if (!p->pinned[0]) {
        for (int i = 0; i < 2; ++i) {
            NW_HIP(hipHostMalloc(&p->pinned[i], kPiece, hipHostMallocDefault));
            NW_HIP(hipEventCreateWithFlags(&p->pinned_ev[i], hipEventDisableTiming));
        }
    }
    const size_t npieces = (bytes + kPiece - 1) / kPiece;
    for (size_t i = 0; i <= npieces; ++i) {
        if (i < npieces) {
            const size_t off = i * kPiece;
            NW_HIP(hipMemcpyAsync(p->pinned[i & 1], src + off, std::min(kPiece, bytes - off), hipMemcpyDeviceToHost,
                                  p->stream));
            NW_HIP(hipEventRecord(p->pinned_ev[i & 1], p->stream));
        }
        if (i > 0) {                                  // piece i-1 landed: copy it out while piece i flies
            const size_t k = i - 1, off = k * kPiece;
            NW_HIP(hipEventSynchronize(p->pinned_ev[k & 1]));
            nw::host::parallel_copy(dst + off, (const char*)p->pinned[k & 1], std::min(kPiece, bytes - off),
                                   copy_threads());
        }
    }
    return NW_OK;
}

}  // namespace

namespace nw {
int dcheck_register(DcheckTake fn) {
    dcheck_registry().push_back(fn);
    return (int)dcheck_registry().size();
}
}  // namespace nw

extern "C" {

const char* nw_last_error(void) { return g_last_error.c_str(); }

const char* nw_version(void) { return "ninwave 0.1.0 (gfx950)"; }

int nw_debug_bounds(void) { return kDebugBounds ? 1 : 0; }

int nw_debug_selftest(int device) {
    if (!kDebugBounds) return fail(NW_E_STATE, "nw_debug_selftest: not the debug library");
    int ndev = 0;
    NW_TRY(nw_device_count(&ndev));
    if (device < 0 || device >= ndev) return fail(NW_E_INVALID, "nw_debug_selftest: device out of range");
    DeviceGuard guard(device);
    NW_TRY(dcheck_collect(nullptr));   // nothing pending from earlier calls
    NW_HIP(nw::launch_dcheck_selftest(nullptr));
    return dcheck_collect(nullptr);
}

int nw_set_log_level(int level) {
    const int prev = log_level();
    g_log_level.store(std::max(0, level));
    return prev;
}

int nw_device_count(int* n) {
    if (!n) return fail(NW_E_INVALID, "nw_device_count: null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(NW_E_NODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *n = c;
    return NW_OK;
}

int nw_trans_grid(double real_length, double sfreq, int interpolate, nw_grid* g) {
    if (!g || !(real_length > 0.0) || !(sfreq > 0.0))
        return fail(NW_E_INVALID, "nw_trans_grid: need real_length > 0, sfreq > 0");
    nw::host::trans_grid(real_length, sfreq, interpolate != 0, &g->delta, &g->len_valid, &g->len_full);
    return NW_OK;
}

int nw_fused_supported(int64_t n, int dtype) {
    return nw::fused_supported(n, dtype) || nw::large_supported(n, dtype) || nw::chirp_supported(n, dtype) ? 1 : 0;
}

int nw_decim_supported(int64_t n, int dtype, int decim) { return nw::decim_supported(n, dtype, decim) ? 1 : 0; }

int nw_plan_set_decim(nw_plan* p, int decim) {
    if (!p) return fail(NW_E_INVALID, "nw_plan_set_decim: null plan");
    if (p->executed) return fail(NW_E_STATE, "nw_plan_set_decim: call it before the first execute");
    if (decim == 1) {
        p->decim = 1;
        return NW_OK;
    }
    if (!nw::decim_supported(p->n, p->dtype, decim))
        return fail(NW_E_INVALID, "nw_plan_set_decim: decim " + std::to_string(decim) + " is not supported at n " +
                                      std::to_string(p->n) + " (nw_decim_supported: power-of-two n 2048 .. 16384, "
                                      "power-of-two decim with n / decim >= 1024)");
    if (p->form != FORM_ONE_PASS)
        return fail(NW_E_INVALID, "nw_plan_set_decim: the rocFFT engine does not decimate (slice its full result)");
    p->decim = decim;
    nw_logf(1, "plan %p: decim %d: rows of %lld samples from the folded spectrum (nw_fused_decim_kernel)", (void*)p,
            decim, (long long)p->n_out());
    return NW_OK;
}

int nw_plan_create(nw_plan** out, int device, int64_t n, int64_t max_batch, int32_t nfreq, int dtype,
                   uint32_t flags) {
    if (!out) return fail(NW_E_INVALID, "nw_plan_create: null plan pointer");
    *out = nullptr;
    if (n < 1 || max_batch < 1 || nfreq < 1) return fail(NW_E_INVALID, "nw_plan_create: n, max_batch, nfreq must be >= 1");
    if (dtype != NW_F32 && dtype != NW_F64) return fail(NW_E_INVALID, "nw_plan_create: dtype must be NW_F32 or NW_F64");
    if ((flags & NW_ENGINE_ROCFFT) && (flags & NW_ENGINE_FUSED))
        return fail(NW_E_INVALID, "nw_plan_create: choose one engine");
    int ndev = 0;
    NW_TRY(nw_device_count(&ndev));
    if (ndev == 0) return fail(NW_E_NODEVICE, "nw_plan_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(NW_E_INVALID, "nw_plan_create: device out of range");
    std::call_once(g_rocfft_once, [] { rocfft_setup(); });

    DeviceGuard guard(device);
    std::unique_ptr<nw_plan> p(new nw_plan());   // an early return frees what it holds by then
    p->device = device;
    p->n = n;
    p->nh = n / 2 + 1;
    p->max_batch = max_batch;
    p->nfreq = nfreq;
    p->dtype = dtype;
    p->flags = flags;
    p->esz = dtype == NW_F32 ? 4 : 8;
    const bool large_ok = !nw::fused_supported(n, dtype) && nw::large_supported(n, dtype);
    const bool chirp_sure = nw::chirp_supported(n, dtype) && !(flags & NW_NO_CHIRP);
    // 2n - 1 > M_max: the chirp-z form only if the auto engine finds every row narrow enough
    const bool chirp_maybe = !chirp_sure && !large_ok && nw::chirp_possible(n, dtype) && !(flags & NW_NO_CHIRP) &&
                             !(flags & (NW_ENGINE_ROCFFT | NW_ENGINE_FUSED));
    const bool fused_ok = nw::fused_supported(n, dtype) || large_ok || chirp_sure;
    if ((flags & NW_ENGINE_FUSED) && !fused_ok)
        return fail(NW_E_INVALID, "nw_plan_create: fused engine does not support this n/dtype");
    const bool fused = (flags & NW_ENGINE_FUSED) || (!(flags & NW_ENGINE_ROCFFT) && (fused_ok || chirp_maybe));
    p->form = !fused ? FORM_ROCFFT
              : large_ok ? FORM_TWO_PASS
              : (chirp_sure || chirp_maybe) ? FORM_CHIRP : FORM_ONE_PASS;
    p->chirp_tentative = fused && chirp_maybe;
    hipError_t e = hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(NW_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    p->stream = p->own_stream;
    if (rocfft_execution_info_create(&p->info) != rocfft_status_success)
        return fail(NW_E_ROCFFT, "rocfft_execution_info_create failed");
    NW_TRY(p->d_x.ensure((size_t)max_batch * n * p->esz));
    NW_TRY(p->d_X.ensure((size_t)max_batch * p->nh * 2 * p->esz));
    if (p->form == FORM_ONE_PASS) {
        e = nw::fused_prepare(n, dtype);
        if (e != hipSuccess) return fail(NW_E_HIP, std::string("fused_prepare: ") + hipGetErrorString(e));
    }
    nw_logf(1, "plan %p: device %d n %lld nfreq %d %s max_batch %lld: %s engine, %s", (void*)p.get(), device,
            (long long)n, (int)nfreq, dtype_name(dtype), (long long)max_batch, fused ? "fused" : "rocFFT",
            p->form == FORM_ROCFFT ? "rocFFT forward / K1 multiply / rocFFT inverse / K2 epilogue"
            : p->form == FORM_TWO_PASS ? "two-pass form (rows_kernel + cols_kernel)"
            : p->chirp_tentative ? "chirp-z form if every row fits on chip (settled at the first execute)"
            : p->form == FORM_CHIRP ? "chirp-z form (nw_chirp_kernel)" : "one-pass form (fwd_r2c_kernel + nw_fused_kernel)");
    *out = p.release();
    return NW_OK;
}

// WaveletMode.Normal table on the device (MexicanHat / Haar; base.py:249-256) from the host's
// row geometry (nw::host::normal_rows).  Rows of equal length share one batched fp64 rocFFT.
static int build_normal_table(nw_plan* p, int kind, const std::vector<nw::NormalRow>& rows, int64_t lmax, int64_t total,
                              double sigma) {
    const int F = p->nfreq;
    std::map<int64_t, std::vector<int>> by_len;
    for (int f = 0; f < F; ++f) by_len[rows[f].len].push_back(f);
    p->row_len_host.resize(F);
    for (int f = 0; f < F; ++f) p->row_len_host[f] = rows[f].len;
    DevBuf d_rows, d_buf;
    NW_TRY(d_rows.ensure(F * sizeof(nw::NormalRow)));
    NW_TRY(d_buf.ensure((size_t)std::max<int64_t>(total, 1) * 2 * sizeof(double)));
    NW_TRY(p->d_table.ensure(std::max<size_t>((size_t)F * lmax * 2 * p->esz, 16)));
    NW_TRY(p->d_row_len.ensure(F * sizeof(int64_t)));
    NW_HIP(hipMemcpy(d_rows.ptr, rows.data(), F * sizeof(nw::NormalRow), hipMemcpyHostToDevice));
    NW_HIP(hipMemcpy(p->d_row_len.ptr, p->row_len_host.data(), F * sizeof(int64_t), hipMemcpyHostToDevice));
    const nw::NormalRow* dr = (const nw::NormalRow*)d_rows.ptr;
    NW_HIP(nw::launch_normal_time(dr, F, lmax, kind, sigma, d_buf.ptr, p->stream));
    NW_TRY(fft_rows_by_length(rows, by_len, false, d_buf.ptr, p->stream));
    NW_HIP(nw::launch_normal_finish(dr, F, lmax, (p->flags & NW_INTERPOLATE) != 0, d_buf.ptr, p->dtype, p->d_table.ptr,
                                    p->stream));
    NW_HIP(hipStreamSynchronize(p->stream));
    return NW_OK;
}

// Distinct rows of W (see nw_plan::uniq).  A row is a function of (kind, params, grid)
// and, except for Shannon, of its freq (tables: of its contents), so equal freqs (equal
// table rows) give bit-identical outputs.
static int setup_unique_rows(nw_plan* p, int kind, const double* freqs, const void* host_table) {
    const int F = p->nfreq;
    p->stats.unique_rows = F;
    const bool user_table = kind == NW_TABLE && host_table;
    const nw::host::RowGroups groups =
        nw::host::group_rows(kind == NW_SHANNON, F, freqs, user_table ? (const double*)host_table : nullptr,
                             p->desc.len_full, user_table && !p->row_len_host.empty() ? p->row_len_host.data() : nullptr);
    const int U = (int)groups.uniq.size();
    if ((p->flags & NW_NO_DEDUP) || 2 * U > F) return NW_OK;
    NW_TRY(build_row_view(p, p->desc, groups.uniq, groups.packed, &p->uniq));
    p->stats.unique_rows = U;
    return NW_OK;
}

int nw_plan_set_wavelet(nw_plan* p, int kind, const double* params, int nparams, const double* freqs,
                        const nw_grid* grid, const void* table, const int64_t* row_len) {
    if (!p || !freqs || !grid) return fail(NW_E_INVALID, "nw_plan_set_wavelet: null argument");
    if (kind < NW_MORSE || kind > NW_HAAR) return fail(NW_E_INVALID, "nw_plan_set_wavelet: unknown kind");
    const bool normal = kind == NW_MEXICAN_HAT || kind == NW_HAAR;
    if (kind == NW_TABLE && !table) return fail(NW_E_INVALID, "nw_plan_set_wavelet: NW_TABLE needs a table");
    if (grid->len_full < 0 || grid->len_valid < 0 || grid->len_valid > grid->len_full)
        return fail(NW_E_INVALID, "nw_plan_set_wavelet: bad grid lengths");
    const int F = p->nfreq;
    for (int i = 0; i < F; ++i)
        if (kind != NW_TABLE && kind != NW_SHANNON && freqs[i] == 0.0)
            return fail(NW_E_INVALID, "nw_plan_set_wavelet: freq == 0 (ZeroDivisionError in base.py:234-235)");
    if (kind == NW_TABLE && row_len)
        for (int i = 0; i < F; ++i)
            if (row_len[i] < 0 || row_len[i] > grid->len_full)
                return fail(NW_E_INVALID, "nw_plan_set_wavelet: row_len out of range");
    // Normal-mode rows: the geometry mirrors numpy on the host: _setup_waveletshape's span and
    // step (base.py:196-216, real_length = 1, zero_mean), np.arange's length ceil((stop - start)
    // / step) and fill, half = int((sfreq * real_wave_length - m) / 2) zeros per side
    // (base.py:253-254)
    std::vector<nw::NormalRow> nrows;
    int64_t lmax = 0, ntotal = 0;
    double nsigma = 0.0;
    if (normal && !nw::host::normal_rows(kind == NW_MEXICAN_HAT, params, nparams, freqs, F, nrows, &lmax, &ntotal, &nsigma))
        return fail(NW_E_INVALID, "nw_plan_set_wavelet: negative padding (np.zeros of a negative size)");
    nw::WDesc d{};
    d.kind = kind;
    d.nfreq = F;
    d.delta = grid->delta;
    d.len_full = grid->len_full;
    d.len_valid = grid->len_valid;
    std::vector<double> peak(F, 1.0);
    std::vector<float> xstep(F, 0.f);
    if (kind == NW_MORSE || kind == NW_MORLET) {
        const nw::host::StockParams sp = nw::host::stock_params(kind, params, nparams);
        d.b = sp.b, d.r = sp.r, d.b_over_r = sp.b_over_r;
        d.sigma = sp.sigma, d.cpi = sp.cpi, d.kappa = sp.kappa;
    }
    if (kind == NW_MORSE) {
        for (int i = 0; i < F; ++i) xstep[i] = (float)(grid->delta / freqs[i]);
        d.morse_ovf = nw::host::morse_may_overflow(d.b, d.r, grid->delta, grid->len_valid, freqs, F) ? 1 : 0;
    } else if (kind == NW_MORLET) {
        for (int i = 0; i < F; ++i) {
            peak[i] = nw::host::morlet_peak(d.sigma, freqs[i]);
            xstep[i] = (float)(grid->delta / freqs[i] * peak[i]);
        }
    }

    // every argument is good: from here to the end the plan has no wavelet, so a failure (out of
    // memory) leaves it refusing executes rather than running on half of each wavelet
    DeviceGuard guard(p->device);
    p->has_wavelet = false;
    p->wtab_valid = false;
    p->uniq.reset();
    p->over.reset();
    p->row_len_host.clear();
    NW_TRY(p->d_freq.ensure(F * sizeof(double)));
    NW_TRY(p->d_peak.ensure(F * sizeof(double)));
    NW_TRY(p->d_xstep32.ensure(F * sizeof(float)));
    NW_HIP(hipMemcpy(p->d_freq.ptr, freqs, F * sizeof(double), hipMemcpyHostToDevice));
    NW_HIP(hipMemcpy(p->d_peak.ptr, peak.data(), F * sizeof(double), hipMemcpyHostToDevice));
    NW_HIP(hipMemcpy(p->d_xstep32.ptr, xstep.data(), F * sizeof(float), hipMemcpyHostToDevice));
    p->d_table.reset();   // sized to this wavelet (nw_stats.device_bytes)
    p->d_row_len.reset();
    if (normal) {
        NW_TRY(build_normal_table(p, kind, nrows, lmax, ntotal, nsigma));
        kind = NW_TABLE;               // from here on a (device-built) table like any other
        d.kind = NW_TABLE;
        d.delta = 1.0;
        d.len_full = d.len_valid = lmax;
    } else if (kind == NW_TABLE) {
        p->row_len_host.assign(F, grid->len_full);
        if (row_len) p->row_len_host.assign(row_len, row_len + F);
        NW_TRY(p->d_row_len.ensure(F * sizeof(int64_t)));
        NW_HIP(hipMemcpy(p->d_row_len.ptr, p->row_len_host.data(), F * sizeof(int64_t), hipMemcpyHostToDevice));
        if (grid->len_full > 0) {
            const size_t cnt = (size_t)F * grid->len_full;
            const size_t bytes = cnt * 2 * p->esz;
            NW_TRY(p->d_table.ensure(bytes));
            if (p->dtype == NW_F64) {
                NW_HIP(hipMemcpy(p->d_table.ptr, table, bytes, hipMemcpyHostToDevice));
            } else {
                std::vector<float> tmp(cnt * 2);
                const double* src = (const double*)table;
                for (size_t i = 0; i < cnt * 2; ++i) tmp[i] = (float)src[i];
                NW_HIP(hipMemcpy(p->d_table.ptr, tmp.data(), bytes, hipMemcpyHostToDevice));
            }
        }
    }
    d.freq = (const double*)p->d_freq.ptr;
    d.peak = (const double*)p->d_peak.ptr;
    d.xstep32 = (const float*)p->d_xstep32.ptr;
    d.table = p->d_table.ptr;
    d.row_len = (const int64_t*)p->d_row_len.ptr;
    p->desc = d;
    if (p->chirp_tentative) p->form = FORM_CHIRP;   // a new wavelet may fit where the last one did not
    NW_TRY(setup_unique_rows(p, kind, freqs, normal ? nullptr : table));
    p->has_wavelet = true;
    nw_logf(1, "plan %p: wavelet kind %d, %d scales (%s), row length %lld", (void*)p, kind, F,
            p->uniq.U ? (std::to_string(p->uniq.U) + " distinct rows, expanded after the transform").c_str()
                      : "every row distinct",
            (long long)d.len_full);
    return NW_OK;
}

int nw_plan_wavelet_shape(nw_plan* p, int64_t* len_full, int64_t* row_len) {
    if (!p || !len_full) return fail(NW_E_INVALID, "nw_plan_wavelet_shape: null argument");
    if (!p->has_wavelet) return fail(NW_E_STATE, "nw_plan_wavelet_shape: no wavelet attached");
    *len_full = p->desc.len_full;
    if (row_len)
        for (int f = 0; f < p->nfreq; ++f)
            row_len[f] = (p->desc.kind == NW_TABLE && !p->row_len_host.empty()) ? p->row_len_host[f] : p->desc.len_full;
    return NW_OK;
}

int nw_plan_wavelet_rows(nw_plan* p, void* out_host) {
    if (!p || !out_host) return fail(NW_E_INVALID, "nw_plan_wavelet_rows: null argument");
    if (!p->has_wavelet) return fail(NW_E_STATE, "nw_plan_wavelet_rows: no wavelet attached");
    if (p->desc.len_full == 0) return NW_OK;
    DeviceGuard guard(p->device);
    const size_t bytes = (size_t)p->nfreq * p->desc.len_full * p->esz * (p->desc.kind == NW_TABLE ? 2 : 1);
    DevBuf rows;
    NW_TRY(rows.ensure(bytes));
    NW_HIP(nw::launch_rows(p->desc, p->dtype, rows.ptr, p->stream));
    NW_HIP(hipMemcpyAsync(out_host, rows.ptr, bytes, hipMemcpyDeviceToHost, p->stream));
    NW_HIP(hipStreamSynchronize(p->stream));
    return NW_OK;
}

int nw_plan_row_support(nw_plan* p, int method, int32_t* kmax_out) {
    if (!p || !kmax_out) return fail(NW_E_INVALID, "nw_plan_row_support: null argument");
    if (!p->has_wavelet) return fail(NW_E_STATE, "nw_plan_row_support: no wavelet attached");
    if (p->form != FORM_TWO_PASS)
        return fail(NW_E_STATE, "nw_plan_row_support: the plan does not run the two-pass engine");
    if (method != 0 && method != 1) return fail(NW_E_INVALID, "nw_plan_row_support: bad method");
    DeviceGuard guard(p->device);
    // into a scratch buffer (the plan's own support stays as built: under a repeated-rows view
    // it holds the distinct rows only)
    DevBuf tmp;
    NW_TRY(tmp.ensure(nw::large_support_bytes(p->nfreq)));
    NW_HIP(nw::large_row_support(with_geometry(p, p->desc), p->dtype, tmp.ptr, method == 1, p->stream));
    NW_HIP(hipMemcpyAsync(kmax_out, tmp.ptr, (size_t)p->nfreq * sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    NW_HIP(hipStreamSynchronize(p->stream));
    return NW_OK;
}

int nw_execute(nw_plan* p, const void* x, int64_t nsig, void* out, int out_kind, int mem) {
    if (!p || (!x && nsig > 0) || (!out && nsig > 0)) return fail(NW_E_INVALID, "nw_execute: null argument");
    if (!p->has_wavelet) return fail(NW_E_STATE, "nw_execute: nw_plan_set_wavelet first");
    if (!is_execute_kind(out_kind)) return fail(NW_E_INVALID, "nw_execute: bad out_kind");
    if (mem != NW_MEM_HOST && mem != NW_MEM_DEVICE) return fail(NW_E_INVALID, "nw_execute: bad mem");
    if (nsig < 0) return fail(NW_E_INVALID, "nw_execute: nsig < 0");
    if (is_reduction(out_kind) && !out) return fail(NW_E_INVALID, "nw_execute: null out");
    if (nsig == 0 && !is_reduction(out_kind)) return NW_OK;
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));

    nw_logf(1, "plan %p: execute %s, %lld signals, %s buffers", (void*)p, out_name(out_kind), (long long)nsig,
            mem == NW_MEM_HOST ? "host" : "device");
    if (is_reduction(out_kind)) {
        NW_TRY(execute_reduce(p, d, x, nsig, out, out_kind, mem == NW_MEM_HOST));
        return dcheck_collect(p->stream);
    }

    const size_t out_elem = (out_kind == NW_OUT_CWT ? 2 : 1) * p->esz;
    const size_t row_out = (size_t)p->nfreq * p->n_out() * out_elem;  // one signal's output bytes
    const bool host = mem == NW_MEM_HOST;
    // host buffers: the chunk's result on the device before it is read back (rocFFT form, CWT:
    // the complex result is read back straight from d_Y)
    void* staging = nullptr;
    if (host && p->form == FORM_ROCFFT && out_kind == NW_OUT_CWT) {
        NW_TRY(need_Y(p, p->nfreq));
        staging = p->d_Y.ptr;
    } else if (host) {
        NW_TRY(p->d_out.ensure((size_t)p->max_batch * row_out));
        staging = p->d_out.ptr;
    }
    // a page-locked destination (nw_host_alloc) is written by DMA directly (a fresh pageable
    // array the caller allocated may have been advised onto huge pages by it, nw_host_advise;
    // the caller's memory policy is never changed here)
    const bool direct = host && host_pinned(out, (size_t)nsig * row_out);

    for (int64_t s0 = 0; s0 < nsig; s0 += p->max_batch) {
        const int64_t c = std::min<int64_t>(p->max_batch, nsig - s0);
        const char* xs = (const char*)x + (size_t)s0 * p->n * p->esz;
        char* os = (char*)out + (size_t)s0 * row_out;
        if (host) {
            NW_TRY(stage_chunk(p, xs, (size_t)c * p->n * p->esz));
            NW_TRY(run_chunk(p, d, p->d_x.ptr, c, staging, out_kind, true));
            NW_TRY(staged(p, ST_COPY, [&] {
                if (direct) {
                    NW_HIP(hipMemcpyAsync(os, staging, (size_t)c * row_out, hipMemcpyDeviceToHost, p->stream));
                    return NW_OK;
                }
                return copy_out(p, os, (const char*)staging, (size_t)c * row_out);
            }));
            NW_HIP(hipStreamSynchronize(p->stream));
        } else {
            NW_TRY(run_chunk(p, d, xs, c, os, out_kind, true));
        }
        p->stats.chunks++;
    }
    p->stats.executes++;
    if (host) NW_TRY(resolve_timing(p));
    return dcheck_collect(p->stream);
}

int nw_pair_partials_supported(int64_t n, int dtype, int kind, int out_kind) {
    return nw::pair_partials_supported(n, dtype, kind, out_kind) ? 1 : 0;
}

int nw_execute_pair(nw_plan* p, const void* xa, const void* xb, int64_t npairs, void* out, int out_kind, int mem) {
    if (!p || !out || ((!xa || !xb) && npairs > 0)) return fail(NW_E_INVALID, "nw_execute_pair: null argument");
    if (!p->has_wavelet) return fail(NW_E_STATE, "nw_execute_pair: nw_plan_set_wavelet first");
    if (const char* e = conn_kind_error(out_kind, nullptr)) return fail(NW_E_INVALID, std::string("nw_execute_pair: ") + e);
    if (mem != NW_MEM_HOST && mem != NW_MEM_DEVICE) return fail(NW_E_INVALID, "nw_execute_pair: bad mem");
    if (npairs < 0) return fail(NW_E_INVALID, "nw_execute_pair: npairs < 0");
    if (p->max_batch < 2)
        return fail(NW_E_INVALID, "nw_execute_pair: the plan's max_batch must be >= 2 (a chunk holds max_batch / 2 pairs)");
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    nw_logf(1, "plan %p: execute %s, %lld pairs, %s buffers", (void*)p, out_name(out_kind), (long long)npairs,
            mem == NW_MEM_HOST ? "host" : "device");
    NW_TRY(execute_pair(p, d, xa, xb, npairs, out, out_kind, mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_conn_tiles(int32_t nchan, const int32_t* ia, const int32_t* ib, int64_t npairs, int32_t* tile_of_pair,
                  int64_t* ntiles, int32_t* limits) {
    if (!ntiles) return fail(NW_E_INVALID, "nw_conn_tiles: null argument");
    NW_TRY(check_pairs("nw_conn_tiles", nchan, ia, ib, npairs));
    *ntiles = (int64_t)nw::host::conn_tiles(ia, ib, npairs, tile_of_pair).size();
    if (limits) limits[0] = nw::kConnCh, limits[1] = nw::kConnPairs, limits[2] = nw::kConnTileN;
    return NW_OK;
}

int nw_execute_conn(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ia, const int32_t* ib,
                    int64_t npairs, void* out_cross, void* out_power, int out_kind, int mem) {
    NW_TRY(check_epoch_call("nw_execute_conn", p, !p || (!x && nepochs > 0) || (!out_cross && npairs > 0),
                            conn_kind_error(out_kind, out_power), mem, nepochs, nchan, ia, ib, npairs));
    NW_TRY(check_chunk("nw_execute_conn", p, nchan));
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    nw_logf(1, "plan %p: execute conn %s, %lld epochs x %d channels, %lld pairs, %s buffers", (void*)p, out_name(out_kind),
            (long long)nepochs, (int)nchan, (long long)npairs, mem == NW_MEM_HOST ? "host" : "device");
    NW_TRY(execute_conn(p, d, x, nepochs, nchan, ia, ib, npairs, out_cross, out_power, out_kind, mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_conn_time_count(int64_t n_out, int64_t t0, int64_t t1, int64_t step, int64_t* count) {
    if (!count) return fail(NW_E_INVALID, "nw_conn_time_count: null argument");
    NW_TRY(check_window("nw_conn_time_count", n_out, t0, t1, step));
    *count = nw::conn_time_count(t0, t1, step);
    return NW_OK;
}

int nw_execute_conn_time(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ia, const int32_t* ib,
                         int64_t npairs, int64_t t0, int64_t t1, int64_t step, void* out_sum, void* out_power,
                         int out_kind, int mem) {
    const char* const who = "nw_execute_conn_time";
    NW_TRY(check_epoch_call(who, p, !p || (!x && nepochs > 0) || (!out_sum && npairs > 0 && nepochs > 0),
                            conn_kind_error(out_kind, out_power), mem, nepochs, nchan, ia, ib, npairs));
    NW_TRY(check_chunk(who, p, nchan));
    NW_TRY(check_window(who, p->n_out(), t0, t1, step));
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    NW_TRY(execute_conn_time(p, d, x, nepochs, nchan, ia, ib, npairs, t0, t1, step, out_sum, out_power, out_kind,
                             mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_execute_env_time(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ia, const int32_t* ib,
                        int64_t npairs, int64_t t0, int64_t t1, int64_t step, void* out_pair, void* out_chan,
                        int env_kind, int mem) {
    const char* const who = "nw_execute_env_time";
    NW_TRY(check_epoch_call(who, p, !p || (!x && nepochs > 0) || (!out_pair && npairs > 0 && nepochs > 0),
                            env_kind != NW_ENV_PLAIN && env_kind != NW_ENV_ORTH
                                ? "env_kind must be NW_ENV_PLAIN or NW_ENV_ORTH" : nullptr,
                            mem, nepochs, nchan, ia, ib, npairs));
    NW_TRY(check_chunk(who, p, nchan));
    NW_TRY(check_window(who, p->n_out(), t0, t1, step));
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    NW_TRY(execute_env_time(p, d, x, nepochs, nchan, ia, ib, npairs, t0, t1, step, out_pair, out_chan, env_kind,
                            mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_execute_pac(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ip, const int32_t* ia,
                   int64_t npairs, const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam, int64_t t0,
                   int64_t t1, int64_t step, void* out_m, void* out_amp, void* out_phase, int mem) {
    const char* const who = "nw_execute_pac";
    NW_TRY(check_epoch_call(who, p, !p || (!x && nepochs > 0) || (!out_m && npairs > 0 && nepochs > 0 && nph > 0 && nam > 0),
                            nullptr, mem, nepochs, nchan, ip, ia, npairs));
    NW_TRY(check_scale_lists(who, p, fph, nph, fam, nam));
    NW_TRY(check_chunk(who, p, nchan));
    NW_TRY(check_window(who, p->n_out(), t0, t1, step));
    // the grid of one chunk's launch (block indices are 32-bit)
    const int64_t blocks = nw::pac_blocks(std::max<int64_t>(p->max_batch / nchan, 1), npairs, nw::pac_tiles(nph, nam), true);
    if (blocks < 0 || blocks > 0x7fffffff)
        return fail(NW_E_INVALID, "nw_execute_pac: " + std::to_string(npairs) + " pairs x " + std::to_string(nph) + " x " +
                                      std::to_string(nam) + " scales per chunk need more than 2^31 - 1 blocks");
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    NW_TRY(execute_pac(p, d, x, nepochs, nchan, ip, ia, npairs, fph, nph, fam, nam, t0, t1, step, out_m, out_amp,
                       out_phase, mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_execute_pac_surr(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ip, const int32_t* ia,
                        int64_t npairs, const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam, int64_t t0,
                        int64_t t1, int64_t step, const int64_t* lags, int32_t nlags, int centre, void* out_m,
                        void* out_amp, void* out_phase, void* out_stat, void* out_all, int mem) {
    const char* const who = "nw_execute_pac_surr";
    const bool cells = npairs > 0 && nepochs > 0 && nph > 0 && nam > 0;
    NW_TRY(check_epoch_call(who, p, !p || (!x && nepochs > 0) || (!out_m && cells) || (!out_stat && !out_all) ||
                                        (!lags && nlags > 0),
                            centre != NW_PAC_SURR_PLAIN && centre != NW_PAC_SURR_DEBIASED
                                ? "centre must be NW_PAC_SURR_PLAIN or NW_PAC_SURR_DEBIASED" : nullptr,
                            mem, nepochs, nchan, ip, ia, npairs));
    NW_TRY(check_scale_lists(who, p, fph, nph, fam, nam));
    NW_TRY(check_chunk(who, p, nchan));
    NW_TRY(check_window(who, p->n_out(), t0, t1, step));
    const int64_t count = nw::conn_time_count(t0, t1, step);
    if (nlags < 0 || nlags > NW_PAC_MAX_LAGS)
        return fail(NW_E_INVALID, std::string(who) + ": nlags (" + std::to_string(nlags) + ") must lie in [0, " +
                                      std::to_string(NW_PAC_MAX_LAGS) + "]");
    for (int32_t s = 0; s < nlags; ++s)
        if (lags[s] < 0 || lags[s] >= count)
            return fail(NW_E_INVALID, std::string(who) + ": lag " + std::to_string(s) + " = " + std::to_string(lags[s]) +
                                          " is outside [0, " + std::to_string(count) + "), the window's samples");
    // the grids of one chunk's launches (block indices are 32-bit)
    const int64_t per = std::max<int64_t>(p->max_batch / nchan, 1);
    const int64_t blocks = nw::pac_blocks(per, npairs, nw::pac_tiles(nph, nam), true);
    const int64_t stage_blocks = nw::pac_surr_stage_blocks(per * nchan * ((int64_t)nph + nam), count);
    if (blocks < 0 || blocks > 0x7fffffff || stage_blocks > 0x7fffffff)
        return fail(NW_E_INVALID, std::string(who) + ": " + std::to_string(npairs) + " pairs x " + std::to_string(nph) + " x " +
                                      std::to_string(nam) + " scales per chunk need more than 2^31 - 1 blocks");
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    NW_TRY(execute_pac_surr(p, d, x, nepochs, nchan, ip, ia, npairs, fph, nph, fam, nam, t0, t1, step, lags, nlags, centre,
                            out_m, out_amp, out_phase, out_stat, out_all, mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_execute_erpac(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ip, const int32_t* ia,
                     int64_t npairs, const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam, int64_t t0,
                     int64_t t1, int64_t step, void* out_m, void* out_amp, void* out_phase, int mem) {
    const char* const who = "nw_execute_erpac";
    NW_TRY(check_epoch_call(who, p, !p || (!x && nepochs > 0) || (!out_m && npairs > 0 && nph > 0 && nam > 0 && t0 < t1),
                            nullptr, mem, nepochs, nchan, ip, ia, npairs));
    NW_TRY(check_scale_lists(who, p, fph, nph, fam, nam));
    NW_TRY(check_chunk(who, p, nchan));
    NW_TRY(check_window(who, p->n_out(), t0, t1, step));
    // the grid of a launch (block indices are 32-bit): it does not depend on the chunk
    const int64_t blocks = nw::erpac_blocks(npairs, nw::erpac_sample_tiles(nw::conn_time_count(t0, t1, step)),
                                            nw::pac_tiles(nph, nam), true);
    // ... and nw_erpac_rows_kernel's, one thread per (channel, listed scale, sample) of the outputs asked for
    const int64_t row_blocks = ((int64_t)nchan * ((out_amp ? (int64_t)nam : 0) + (out_phase ? (int64_t)nph : 0)) *
                                    nw::conn_time_count(t0, t1, step) + 255) / 256;
    if (blocks < 0 || blocks > 0x7fffffff || row_blocks > 0x7fffffff)
        return fail(NW_E_INVALID, std::string(who) + ": " + std::to_string(npairs) + " pairs x " + std::to_string(nph) + " x " +
                                      std::to_string(nam) + " scales x " + std::to_string(nw::conn_time_count(t0, t1, step)) +
                                      " samples need more than 2^31 - 1 blocks");
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    NW_TRY(execute_erpac(p, d, x, nepochs, nchan, ip, ia, npairs, fph, nph, fam, nam, t0, t1, step, out_m, out_amp,
                         out_phase, mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

int nw_pac_bin_edges(int32_t nbins, double* cs) {
    NW_TRY(check_nbins("nw_pac_bin_edges", nbins));
    if (!cs) return fail(NW_E_INVALID, "nw_pac_bin_edges: null argument");
    pac_bin_edges(nbins, cs);
    return NW_OK;
}

int nw_execute_pac_bins(nw_plan* p, const void* x, int64_t nepochs, int32_t nchan, const int32_t* ip, const int32_t* ia,
                        int64_t npairs, const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam, int64_t t0,
                        int64_t t1, int64_t step, int32_t nbins, void* out_sum, void* out_count, int mem) {
    const char* const who = "nw_execute_pac_bins";
    NW_TRY(check_epoch_call(who, p, !p || (!x && nepochs > 0) || (!out_sum && npairs > 0 && nepochs > 0 && nph > 0 && nam > 0),
                            nullptr, mem, nepochs, nchan, ip, ia, npairs));
    NW_TRY(check_scale_lists(who, p, fph, nph, fam, nam));
    NW_TRY(check_nbins(who, nbins));
    NW_TRY(check_chunk(who, p, nchan));
    NW_TRY(check_window(who, p->n_out(), t0, t1, step));
    // the grid of one chunk's launch (block indices are 32-bit)
    const int64_t blocks = nw::pac_blocks(std::max<int64_t>(p->max_batch / nchan, 1), npairs,
                                          nw::pac_bins_tiles(nph, nam, nbins), true);
    if (blocks < 0 || blocks > 0x7fffffff)
        return fail(NW_E_INVALID, std::string(who) + ": " + std::to_string(npairs) + " pairs x " + std::to_string(nph) + " x " +
                                      std::to_string(nam) + " scales per chunk need more than 2^31 - 1 blocks");
    DeviceGuard guard(p->device);
    nw::WDesc d;
    NW_TRY(begin_execute(p, &d));
    NW_TRY(execute_pac_bins(p, d, x, nepochs, nchan, ip, ia, npairs, fph, nph, fam, nam, t0, t1, step, nbins, out_sum,
                            out_count, mem == NW_MEM_HOST));
    return dcheck_collect(p->stream);
}

}  // extern "C"

namespace {

using nw::host::block_of;   // balanced contiguous blocks, as dist.shard

// A plan is not reentrant: one host thread per plan, so a plan may appear only once.
int check_distinct(nw_plan* const* plans, int nplans, const char* who) {
    for (int i = 0; i < nplans; ++i) {
        if (!plans[i]) return fail(NW_E_INVALID, std::string(who) + ": null plan");
        for (int j = 0; j < i; ++j)
            if (plans[j] == plans[i])
                return fail(NW_E_INVALID, std::string(who) + ": plan " + std::to_string(i) +
                                              " repeats plan " + std::to_string(j) +
                                              " (a plan is not reentrant: create one plan per shard)");
    }
    return NW_OK;
}

// fn(i) for every plan, each on a host thread of its own; the first failure in plan order, as
// "device D: <its message>"
template <typename F>
int on_each_plan(nw_plan* const* plans, int nplans, F&& fn) {
    std::vector<int> rc(nplans, NW_OK);
    std::vector<std::string> err(nplans);
    std::vector<std::thread> th;
    for (int i = 0; i < nplans; ++i)
        th.emplace_back([&, i] {
            rc[i] = fn(i);
            if (rc[i] != NW_OK) err[i] = g_last_error;
        });
    for (auto& t : th) t.join();
    for (int i = 0; i < nplans; ++i)
        if (rc[i] != NW_OK) return fail(rc[i], "device " + std::to_string(plans[i]->device) + ": " + err[i]);
    return NW_OK;
}

// Reductions over devices: each device sums its contiguous block (fp64 partial sums),
// the host adds them in device order, then takes the mean / |mean| exactly as
// k_finalize does.
int execute_multi_reduce(nw_plan* const* plans, int nplans, const void* x, int64_t nsig, void* out, int out_kind) {
    const nw_plan* p0 = plans[0];
    const bool phase = is_phase(out_kind);
    const int64_t fn = (int64_t)p0->nfreq * p0->n_out();
    const size_t comps = (size_t)fn * (phase ? 2 : 1);
    const size_t x_row = (size_t)p0->n * p0->esz;
    std::vector<std::vector<double>> part(nplans);
    NW_TRY(on_each_plan(plans, nplans, [&](int i) {
        int64_t s0 = 0, cnt = 0;
        block_of(nsig, i, nplans, &s0, &cnt);
        if (cnt <= 0) return (int)NW_OK;
        part[i].assign(comps, 0.0);
        return nw_execute(plans[i], (const char*)x + s0 * x_row, cnt, part[i].data(),
                          phase ? NW_OUT_PHASE_SUM : NW_OUT_POWER_SUM, NW_MEM_HOST);
    }));
    std::vector<double> tot(comps, 0.0);
    for (int i = 0; i < nplans; ++i)
        for (size_t j = 0; j < part[i].size(); ++j) tot[j] += part[i][j];
    if (out_kind == NW_OUT_POWER_SUM || out_kind == NW_OUT_PHASE_SUM) {
        std::memcpy(out, tot.data(), comps * sizeof(double));
        return NW_OK;
    }
    const double d = (double)nsig;
    for (int64_t j = 0; j < fn; ++j) {
        const double v = phase ? std::hypot(tot[2 * j] / d, tot[2 * j + 1] / d) : tot[j] / d;
        if (p0->dtype == NW_F32)
            static_cast<float*>(out)[j] = (float)v;
        else
            static_cast<double*>(out)[j] = v;
    }
    return NW_OK;
}

// nw_execute_multi_device reductions, on device 0: gather every device's fp64 partial sums
// peer-to-peer, add them in device order into plan 0's and finalise into out0.
int reduce_partials(nw_plan* const* plans, int nplans, int out_kind, int64_t total, void* out0) {
    nw_plan* p0 = plans[0];
    const bool phase = is_phase(out_kind);
    const int64_t fn = (int64_t)p0->nfreq * p0->n_out();
    const int64_t comps = fn * (phase ? 2 : 1);
    const size_t acc_bytes = (size_t)comps * sizeof(double);
    DeviceGuard g(p0->device);
    double* acc = (double*)p0->d_part.ptr;
    if (nplans > 1) NW_TRY(p0->d_gather.ensure(acc_bytes));
    for (int i = 1; i < nplans; ++i) {
        NW_HIP(hipMemcpyPeerAsync(p0->d_gather.ptr, p0->device, plans[i]->d_part.ptr, plans[i]->device, acc_bytes,
                                  p0->stream));
        NW_HIP(nw::launch_add_f64(acc, (const double*)p0->d_gather.ptr, comps, p0->stream));
    }
    if (out_kind == NW_OUT_POWER_SUM || out_kind == NW_OUT_PHASE_SUM)
        NW_HIP(hipMemcpyAsync(out0, acc, acc_bytes, hipMemcpyDeviceToDevice, p0->stream));
    else
        NW_HIP(nw::launch_finalize(p0->dtype, phase, acc, out0, fn, total, p0->stream));
    NW_HIP(hipStreamSynchronize(p0->stream));
    return NW_OK;
}

// scale_slices: the plans of nw_execute_multi_scales hold slices of one scale list, so their nfreq is
// free, and they mask the same half of the spectrum
int check_same_config(nw_plan* const* plans, int nplans, const char* who, bool scale_slices = false) {
    for (int i = 1; i < nplans; ++i)
        if (plans[i]->n != plans[0]->n || plans[i]->dtype != plans[0]->dtype ||
            (scale_slices ? (plans[i]->flags & NW_INTERPOLATE) != (plans[0]->flags & NW_INTERPOLATE)
                          : plans[i]->nfreq != plans[0]->nfreq))
            return fail(NW_E_INVALID, std::string(who) + (scale_slices ? ": plans must share n, dtype and interpolate"
                                                                       : ": plans must share n, nfreq and dtype"));
    for (int i = 1; i < nplans; ++i)
        if (plans[i]->decim != plans[0]->decim)
            return fail(NW_E_INVALID, std::string(who) + ": plans must share decim");
    return NW_OK;
}

}  // namespace

extern "C" {

int nw_execute_multi(nw_plan* const* plans, int nplans, const void* x, int64_t nsig, void* out, int out_kind) {
    if (!plans || nplans < 1) return fail(NW_E_INVALID, "nw_execute_multi: no plans");
    NW_TRY(check_distinct(plans, nplans, "nw_execute_multi"));
    NW_TRY(check_same_config(plans, nplans, "nw_execute_multi"));
    const nw_plan* p0 = plans[0];
    if (!is_execute_kind(out_kind)) return fail(NW_E_INVALID, "nw_execute_multi: bad out_kind");
    if (nsig < 0) return fail(NW_E_INVALID, "nw_execute_multi: nsig < 0");
    if (is_reduction(out_kind)) return execute_multi_reduce(plans, nplans, x, nsig, out, out_kind);
    const size_t x_row = (size_t)p0->n * p0->esz;
    const size_t o_row = (size_t)p0->nfreq * p0->n_out() * (out_kind == NW_OUT_CWT ? 2 : 1) * p0->esz;
    return on_each_plan(plans, nplans, [&](int i) {
        int64_t s0 = 0, cnt = 0;
        block_of(nsig, i, nplans, &s0, &cnt);
        if (cnt <= 0) return (int)NW_OK;
        return nw_execute(plans[i], (const char*)x + s0 * x_row, cnt, (char*)out + s0 * o_row, out_kind, NW_MEM_HOST);
    });
}

// Device-resident sharding (one process, one host thread per device).  Plan i
// transforms its own device-resident block x[i] (nsig[i] signals) into out[i]; nothing
// crosses PCIe.  Reductions: every device sums its block into fp64 partials, device 0
// gathers them peer-to-peer, adds them in device order and finalises into out[0].
int nw_execute_multi_device(nw_plan* const* plans, int nplans, const void* const* x, const int64_t* nsig,
                            void* const* out, int out_kind) {
    if (!plans || nplans < 1 || !x || !nsig || !out) return fail(NW_E_INVALID, "nw_execute_multi_device: null argument");
    NW_TRY(check_distinct(plans, nplans, "nw_execute_multi_device"));
    NW_TRY(check_same_config(plans, nplans, "nw_execute_multi_device"));
    if (!is_execute_kind(out_kind)) return fail(NW_E_INVALID, "nw_execute_multi_device: bad out_kind");
    int64_t total = 0;
    for (int i = 0; i < nplans; ++i) {
        if (nsig[i] < 0) return fail(NW_E_INVALID, "nw_execute_multi_device: nsig < 0");
        total += nsig[i];
    }
    const bool reduce = is_reduction(out_kind);
    if (reduce && !out[0]) return fail(NW_E_INVALID, "nw_execute_multi_device: null out[0]");
    const bool phase = is_phase(out_kind);
    // reductions: per-device fp64 partial sums (each plan's d_part), then device 0's gather
    // buffer (plans[0]->d_gather); both persist on the plans and are freed with them
    if (reduce) {
        const size_t acc_bytes = (size_t)plans[0]->nfreq * plans[0]->n_out() * (phase ? 2 : 1) * sizeof(double);
        for (int i = 0; i < nplans; ++i) {
            DeviceGuard g(plans[i]->device);
            const int r = plans[i]->d_part.ensure(acc_bytes);
            if (r != NW_OK) return fail(r, "device " + std::to_string(plans[i]->device) +
                                                ": nw_execute_multi_device: partial-sum buffer: " + g_last_error);
        }
    }
    NW_TRY(on_each_plan(plans, nplans, [&](int i) {
        nw_plan* p = plans[i];
        NW_TRY(nw_execute(p, x[i], nsig[i], reduce ? p->d_part.ptr : out[i],
                          reduce ? (phase ? NW_OUT_PHASE_SUM : NW_OUT_POWER_SUM) : out_kind, NW_MEM_DEVICE));
        return nw_plan_sync(p);
    }));
    return reduce ? reduce_partials(plans, nplans, out_kind, total, out[0]) : NW_OK;
}

int nw_execute_multi_scales(nw_plan* const* plans, int nplans, const void* x, int64_t nsig, void* out,
                            int out_kind) {
    if (!plans || nplans < 1 || !plans[0]) return fail(NW_E_INVALID, "nw_execute_multi_scales: no plans");
    NW_TRY(check_distinct(plans, nplans, "nw_execute_multi_scales"));
    NW_TRY(check_same_config(plans, nplans, "nw_execute_multi_scales", true));
    const nw_plan* p0 = plans[0];
    if (!is_execute_kind(out_kind)) return fail(NW_E_INVALID, "nw_execute_multi_scales: bad out_kind");
    if (nsig < 0) return fail(NW_E_INVALID, "nw_execute_multi_scales: nsig < 0");
    if (nsig > 0 && (!x || !out)) return fail(NW_E_INVALID, "nw_execute_multi_scales: null argument");
    int64_t F = 0;
    std::vector<int64_t> f0(nplans);
    for (int i = 0; i < nplans; ++i) {
        f0[i] = F;
        F += plans[i]->nfreq;
    }
    // bytes of one output element: reductions keep their own types (include/ninwave.h)
    size_t oe = (out_kind == NW_OUT_CWT ? 2 : 1) * p0->esz;
    if (out_kind == NW_OUT_POWER_SUM) oe = sizeof(double);
    if (out_kind == NW_OUT_PHASE_SUM) oe = 2 * sizeof(double);
    const size_t x_row = (size_t)p0->n * p0->esz, o_scale = (size_t)p0->n_out() * oe;
    return on_each_plan(plans, nplans, [&](int i) {
        nw_plan* p = plans[i];
        if (is_reduction(out_kind) || nsig <= 1)   // the rows are contiguous in out
            return nw_execute(p, x, nsig, (char*)out + f0[i] * o_scale, out_kind, NW_MEM_HOST);
        for (int64_t s = 0; s < nsig; ++s)
            NW_TRY(nw_execute(p, (const char*)x + s * x_row, 1, (char*)out + ((size_t)s * F + f0[i]) * o_scale, out_kind,
                              NW_MEM_HOST));
        return (int)NW_OK;
    });
}

int nw_baseline(int device, int dtype, const void* x, int64_t count, int64_t row_len, int64_t row0, int64_t row1,
                int op, void* out, int mem, double* stats) {
    if (dtype != NW_F32 && dtype != NW_F64) return fail(NW_E_INVALID, "nw_baseline: dtype must be NW_F32 or NW_F64");
    if (op < NW_BL_MEAN || op > NW_BL_ZLOG) return fail(NW_E_INVALID, "nw_baseline: unknown op");
    if (mem != NW_MEM_HOST && mem != NW_MEM_DEVICE) return fail(NW_E_INVALID, "nw_baseline: bad mem");
    if (count < 0 || row_len < 1 || row0 < 0 || row1 < row0 || row1 > count / row_len)
        return fail(NW_E_INVALID, "nw_baseline: baseline rows out of range");
    if (count > 0 && (!x || !out)) return fail(NW_E_INVALID, "nw_baseline: null array");
    int ndev = 0;
    NW_TRY(nw_device_count(&ndev));
    if (device < 0 || device >= ndev) return fail(NW_E_INVALID, "nw_baseline: device out of range");
    DeviceGuard guard(device);
    const size_t esz = dtype == NW_F32 ? sizeof(float) : sizeof(double);
    const size_t bytes = (size_t)count * esz;
    const bool staged_io = mem == NW_MEM_HOST && bytes;   // host arrays go through device copies
    DevBuf work, d_in, d_res;
    NW_TRY(work.ensure(nw::BL_WORK_DOUBLES * sizeof(double)));
    const void* dx = x;
    void* dout = out;
    if (staged_io) {
        NW_TRY(d_in.ensure(bytes));
        NW_TRY(d_res.ensure(bytes));
        NW_HIP(hipMemcpy(d_in.ptr, x, bytes, hipMemcpyHostToDevice));
        dx = d_in.ptr;
        dout = d_res.ptr;
    }
    NW_HIP(nw::launch_baseline(dtype, dx, count, row0 * row_len, row1 * row_len, op, dout, (double*)work.ptr, nullptr));
    NW_HIP(hipStreamSynchronize(nullptr));
    if (staged_io) NW_HIP(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    if (stats)
        NW_HIP(hipMemcpy(stats, (double*)work.ptr + (nw::BL_WORK_DOUBLES - 2), 2 * sizeof(double), hipMemcpyDeviceToHost));
    return dcheck_collect(nullptr);
}

int nw_make_wavelets(int device, int kind, const double* params, int nparams, const double* freqs, int nfreq,
                     double sfreq, double rwl, void* out, int64_t* max_len, int64_t* row_len) {
    const bool reverse = kind == NW_MORSE || kind == NW_SHANNON;
    if (!reverse && kind != NW_MORLET && kind != NW_MEXICAN_HAT && kind != NW_HAAR)
        return fail(NW_E_INVALID, "nw_make_wavelets: kind must be a stock wavelet");
    if (nfreq < 0 || (nfreq > 0 && !freqs) || !max_len || !row_len) return fail(NW_E_INVALID, "nw_make_wavelets: null argument");
    if (!(sfreq > 0.0)) return fail(NW_E_INVALID, "nw_make_wavelets: sfreq must be > 0");
    const nw::host::StockParams sp = nw::host::stock_params(kind, params, nparams);
    const nw::WaveParams wp{kind, sp.b, sp.r, sp.b_over_r, sp.sigma, sp.cpi, sp.kappa};
    std::vector<nw::WaveRow> rows(nfreq);
    std::map<int64_t, std::vector<int>> by_m;
    int64_t lmax = 0, off = 0;
    for (int f = 0; f < nfreq; ++f) {
        const double fr = freqs[f];
        if (fr == 0.0) return fail(NW_E_INVALID, "nw_make_wavelets: freq == 0 (ZeroDivisionError, base.py:347-348)");
        nw::WaveRow r{};
        if (reverse) {                        // _setup_trans_shape(freq, real_wave_length), base.py:191-194
            const double one = 1.0 / fr;
            r.m = nw::host::arange_len(sfreq / fr * rwl, one);
            r.len = 2 * (r.m / 2);
            r.t0 = 0.0;
            r.delta = one;
            r.t1 = one;
            by_m[r.m].push_back(f);
        } else {                              // _setup_waveletshape(freq, 1, zero_mean=True), base.py:211-216
            const double peak = kind == NW_MORLET ? nw::host::morlet_peak(wp.sigma, fr)
                                : kind == NW_MEXICAN_HAT ? std::sqrt(6.0) / M_PI / M_PI : 1.0;
            const double total = 1.0 / peak * fr * 2.0 * M_PI;
            const double one = 1.0 / sfreq * 2.0 * M_PI * fr / peak;
            r.t0 = -total / 2.0;
            r.m = nw::host::arange_len_from(r.t0, total / 2.0, one);
            r.len = r.m;
            r.t1 = r.t0 + one;
            r.delta = r.t1 - r.t0;
        }
        row_len[f] = r.len;
        lmax = std::max(lmax, r.len);
        rows[f] = r;
    }
    for (auto& kv : by_m)
        for (int f : kv.second) {
            rows[f].off = off;
            off += kv.first;
        }
    *max_len = lmax;
    if (!out || nfreq == 0 || lmax == 0) {
        if (out && nfreq > 0) std::memset(out, 0, (size_t)nfreq * lmax * 16);
        return NW_OK;
    }
    int ndev = 0;
    NW_TRY(nw_device_count(&ndev));
    if (device < 0 || device >= ndev) return fail(NW_E_INVALID, "nw_make_wavelets: device out of range");
    std::call_once(g_rocfft_once, [] { rocfft_setup(); });
    DeviceGuard guard(device);
    const size_t obytes = (size_t)nfreq * lmax * 16;
    DevBuf d_rows, d_buf, d_out;
    NW_TRY(d_rows.ensure(nfreq * sizeof(nw::WaveRow)));
    NW_TRY(d_out.ensure(obytes));
    NW_HIP(hipMemcpy(d_rows.ptr, rows.data(), nfreq * sizeof(nw::WaveRow), hipMemcpyHostToDevice));
    const nw::WaveRow* dr = (const nw::WaveRow*)d_rows.ptr;
    if (!reverse) {
        NW_HIP(nw::launch_wavelet_time(dr, nfreq, lmax, wp, d_out.ptr, nullptr));
    } else {
        NW_TRY(d_buf.ensure((size_t)std::max<int64_t>(off, 1) * 16));
        NW_HIP(nw::launch_wavelet_spectra(dr, nfreq, wp, d_buf.ptr, nullptr));
        NW_TRY(fft_rows_by_length(rows, by_m, true, d_buf.ptr, nullptr));
        NW_HIP(nw::launch_wavelet_pack(dr, nfreq, lmax, d_buf.ptr, d_out.ptr, nullptr));
    }
    NW_HIP(hipDeviceSynchronize());
    NW_HIP(hipMemcpy(out, d_out.ptr, obytes, hipMemcpyDeviceToHost));
    return dcheck_collect(nullptr);
}

int nw_plan_set_stream(nw_plan* p, void* stream) {
    if (!p) return fail(NW_E_INVALID, "nw_plan_set_stream: null plan");
    p->stream = stream ? (hipStream_t)stream : p->own_stream;
    return NW_OK;
}

int nw_plan_get_stream(nw_plan* p, void** stream) {
    if (!p || !stream) return fail(NW_E_INVALID, "nw_plan_get_stream: null argument");
    *stream = (void*)p->stream;
    return NW_OK;
}

int nw_host_alloc(int64_t bytes, void** ptr) {
    if (!ptr || bytes <= 0) return fail(NW_E_INVALID, "nw_host_alloc: bad argument");
    *ptr = nullptr;
    NW_HIP(hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault));
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_bufs[(uintptr_t)*ptr] = (size_t)bytes;
    return NW_OK;
}

int nw_host_advise(void* ptr, int64_t bytes, int64_t* advised) {
    if (!ptr || bytes < 0) return fail(NW_E_INVALID, "nw_host_advise: bad argument");
    const size_t a = nw::host::advise_output(reinterpret_cast<char*>(ptr), (size_t)bytes);
    if (advised) *advised = (int64_t)a;
    return NW_OK;
}

int nw_host_free(void* ptr) {
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_bufs.find((uintptr_t)ptr);
        if (it == g_host_bufs.end()) return fail(NW_E_INVALID, "nw_host_free: not an nw_host_alloc pointer");
        g_host_bufs.erase(it);
    }
    NW_HIP(hipHostFree(ptr));
    return NW_OK;
}

int nw_plan_sync(nw_plan* p) {
    if (!p) return fail(NW_E_INVALID, "nw_plan_sync: null plan");
    DeviceGuard guard(p->device);
    NW_HIP(hipStreamSynchronize(p->stream));
    NW_TRY(resolve_timing(p));
    return dcheck_collect(p->stream);
}

int nw_plan_stats(nw_plan* p, nw_stats* s) {
    if (!p || !s) return fail(NW_E_INVALID, "nw_plan_stats: null argument");
    DeviceGuard guard(p->device);
    NW_TRY(resolve_timing(p));
    *s = p->stats;
    s->engine = p->form == FORM_ROCFFT ? NW_ENGINE_ROCFFT : NW_ENGINE_FUSED;
    s->device_bytes = (int64_t)p->device_bytes();
    return NW_OK;
}

int nw_plan_reset_stats(nw_plan* p) {
    if (!p) return fail(NW_E_INVALID, "nw_plan_reset_stats: null plan");
    DeviceGuard guard(p->device);
    NW_TRY(resolve_timing(p));
    const int64_t uniq = p->stats.unique_rows, kernel = p->stats.kernel, path = p->stats.reduce_path;
    p->stats = nw_stats{};
    p->stats.unique_rows = uniq;
    p->stats.kernel = kernel;
    p->stats.reduce_path = path;
    return NW_OK;
}

int nw_plan_destroy(nw_plan* p) {
    if (!p) return NW_OK;
    DeviceGuard guard(p->device);
    (void)hipStreamSynchronize(p->stream);
    delete p;
    return NW_OK;
}

}  // extern "C"
