// mcgp_hip.hip -- C-ABI (include/mcgp.h) over the gfx950 race kernel.
//
// Host side of the drop-in boundary: validates arguments, folds the reference's
// per-race constants into the kernel's parameter block, owns one cached context
// per HIP device (parameter buffer, scratch histogram, events, the workspace of
// the blocking calls) and launches race_kernel.  No CPU compute path exists here:
// without a HIP device every compute entry point returns MCGP_E_NO_DEVICE.
#include "../../include/mcgp.h"
#include "params_build.h"
#include "race_kernel.hip.h"
#include "race_kernel_reg.hip.h"
#include "championship.hip.h"
#include "champ_rounds.hip.h"
#include "matchups.hip.h"
#include "resume.hip.h"
#include "trace.hip.h"
#include "strategy.hip.h"
#include "gaps.hip.h"
#include "pit_window.hip.h"
#include "conditions.hip.h"
#include "stints.hip.h"
#include "moves.hip.h"
#include "fastest.hip.h"
#include "champ_bonus.hip.h"
#include "champ_given.hip.h"
#include "plan_pack.h"
#include "penalty_pack.h"
#include "pace_pack.h"
#include "event_pack.h"
#include "weather_pack.h"
#include "prior_pack.h"
#include "grid_pack.h"
#include "scenario.hip.h"
#include "champ_pack.h"

#define MCGP_FE_FN __host__ __device__ static inline
#include "frontend_exp.h"
#include "elo_update.h"
#include "normal53_table.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? MCGP_E_NOMEM : MCGP_E_HIP,                    \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

// Field sizes with a register-resident instantiation: every n the ABI admits (1..32).  The generic LDS kernel
// (race_kernel.hip.h) is kept as an independently written second implementation, selected with
// MCGP_FORCE_GENERIC=1: tests run both and require identical results.
#define MCGP_REG_SIZES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) \
    X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// Grid-probability front end (reference src/elo.py:124-141, src/predictor.py:321-407): one thread per driver row.
// in = [rating | teammate_delta | form_score | circuit_affinity], n doubles each.  Thread 0 computes the n pole
// probabilities (a sequential softmax + renormalisation in the reference's order), then every thread builds its
// row.  out may point straight into a parameter block's grid_probs slot.
__global__ void __launch_bounds__(mcgp::kMaxCars)
grid_probs_kernel(const double *__restrict__ in, const int32_t *__restrict__ penalty, int n, double *__restrict__ out)
{
    __shared__ double pole[mcgp::kMaxCars];
    if (threadIdx.x == 0) mcgp_fe_pole_probs(in, in + n, n, pole);
    __syncthreads();
    const int d = threadIdx.x;
    if (d < n) {
        double row[mcgp::kMaxCars], tmp[mcgp::kMaxCars];
        mcgp_fe_grid_row(pole[d], in[2 * n + d], in[3 * n + d], penalty[d], n, row, tmp);
        for (int s = 0; s < n; ++s) out[(size_t)d * n + s] = row[s];
    }
}

// A season of Elo updates (reference src/elo.py:45-122) in one block of 32 x 32 threads with the ratings in LDS.
// Per event: thread (a, b) computes the term of entry a against entry b (csrc/elo_update.h; the one expensive part,
// a 10^x and a division, all m (m - 1) of them at once); a barrier; thread (a, 0) adds entry a's terms up in list
// order -- the reference's inner loop, so the sum has its bits --; a barrier; the deltas are applied.
__global__ void __launch_bounds__(mcgp::kMaxCars * mcgp::kMaxCars)
elo_season_kernel(int n, int n_events, const int32_t *__restrict__ kind, const double *__restrict__ k,
                  const uint32_t *__restrict__ count, const uint8_t *__restrict__ who, const double *__restrict__ value,
                  double *__restrict__ ratings, double *__restrict__ after)
{
    constexpr int M = mcgp::kMaxCars;
    __shared__ double r[2 * M];                           // [kind][driver], row stride n
    __shared__ double term[M][M + 1];
    __shared__ double v[M];
    __shared__ uint8_t w[M];
    const int t = threadIdx.x, a = t / M, b = t % M;
    if (t < 2 * n) r[t] = ratings[t];
    __syncthreads();
    for (int e = 0; e < n_events; ++e) {
        const int m = (int)count[e];
        double *row = r + (kind[e] ? n : 0);
        if (t < m) {
            w[t] = who[(size_t)e * n + t];
            v[t] = value[(size_t)e * n + t];
        }
        __syncthreads();
        if (m >= 2 && a < m && b < m && a != b) term[a][b] = mcgp_elo_term(row[w[a]], v[a], row[w[b]], v[b], k[e], m);
        __syncthreads();
        if (m >= 2 && b == 0 && a < m) {
            double delta = 0.0;
            for (int j = 0; j < m; ++j)
                if (j != a) delta = delta + term[a][j];
            row[w[a]] = row[w[a]] + delta;                // (the terms were all computed from the ratings before the event)
        }
        __syncthreads();
        if (after && t < 2 * n) after[(size_t)e * 2 * n + t] = r[t];
    }
    if (t < 2 * n) ratings[t] = r[t];
}

constexpr int kParamSlots = 4;
constexpr int kSlotReaders = 8;        // streams with a launch in flight on one parameter block
constexpr int kStreamTimers = 8;       // streams whose most recent call keeps its own timing events
constexpr int kCallTimer = -2;         // DeviceCtx::last_timer after a call of several kernels: the call's own pair of events

// Device memory that grows on demand and never shrinks: reserve() reallocates, without keeping the contents, only when it
// is asked for more than it holds.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int reserve(size_t want)
    {
        if (want <= bytes) return MCGP_OK;
        release();
        HIP_TRY(hipMalloc(&p, want));
        bytes = want;
        return MCGP_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T = unsigned char> T *at(size_t offset = 0) const
    {
        return reinterpret_cast<T *>(static_cast<unsigned char *>(p) + offset);
    }
};

struct DeviceCtx {
    std::mutex mu;
    bool ready = false;
    int cu_count = 0;
    size_t lds_per_block = 0;
    // Parameter blocks: a small ring so that a launch never rewrites a block an
    // earlier, still running launch reads; an unchanged problem re-uses its block
    // with no upload at all (bench.py's steady state).
    // Behind each block, in the same allocation, sits the retirement table of its problem (kRetireTabOffset,
    // race_common.hip.h): a function of the block's bytes, built when the block is and uploaded in the same copy, so a
    // block that is re-used brings the table of exactly its rates and laps.
    struct Slot {
        mcgp::KParams *dev = nullptr;
        mcgp::KParams *host = nullptr;        // pinned copy of what `dev` holds
        // one completion event per STREAM that has launched on this block: eviction waits for every one of
        // them (a single event re-recorded by the latest stream would forget a reader still running elsewhere)
        struct Reader {
            hipStream_t stream = nullptr;
            hipEvent_t done = nullptr;        // recorded after that stream's last launch reading `dev`
            bool live = false;
            uint64_t seq = 0;                 // order of the last launch through this entry
        } reader[kSlotReaders];
        hipEvent_t uploaded = nullptr;        // recorded after the upload of `dev`; other streams wait on it
        hipStream_t upload_stream = nullptr;
        bool used = false;
        bool shareable = false;               // false: the device copy differs from `host` (matrix written by the front end)
    } slot[kParamSlots];
    int next_slot = 0;
    unsigned long long *d_hist = nullptr;     // scratch for the host-buffer entry points
    uint8_t *d_grid = nullptr;                // fixed grid for mcgp_simulate_race
    uint8_t *d_order1 = nullptr;              // one finishing order (mcgp_simulate_race)
    double *d_fe_in = nullptr;                // front end: 4 x 32 doubles in, 32 penalties, n x n matrix out
    int32_t *d_fe_pen = nullptr;
    double *d_fe_out = nullptr;
    double *d_norm53 = nullptr;               // binary64 inverse-normal table of the reference-width build (50 KB)
    // timing events per stream (most recent call on that stream), so that calls on different streams of one
    // device do not re-record each other's events
    struct Timer {
        hipStream_t stream = nullptr;
        hipEvent_t start = nullptr, stop = nullptr;
        uint32_t *d_ticket = nullptr;       // the work counter of this stream's launches (race_kernel_reg.hip.h, phase 2)
        DevBuf retire;                      // the lanes' retirement lists of this stream's launches
        bool used = false;
        uint64_t seq = 0;
    } timer[kStreamTimers];
    uint64_t timer_seq = 0;
    int last_timer = -1;
    hipEvent_t call_start = nullptr, call_stop = nullptr;     // the timing events of the last call of several kernels
    // The workspace of every entry point but mcgp_run_device: parameter block, inputs, staging and counts of one call,
    // in regions the call lays out (Layout).  Those calls run on the null stream and hold `mu` throughout, so that a
    // call's work on it is ordered behind all of the previous call's; a grown buffer is replaced through hipFree, which
    // waits for the device.
    DevBuf work;
    uint32_t last_grid = 0, last_block = 0, last_lds = 0;
    char last_kernel[48] = "";
};

constexpr int kMaxDevices = 64;
DeviceCtx g_ctx[kMaxDevices];

int device_count_nothrow()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Validates the device index and returns its context; nothing is initialised yet.
int find_ctx(int device, DeviceCtx **out)
{
    const int nd = device_count_nothrow();
    if (nd <= 0) return fail(MCGP_E_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= nd || device >= kMaxDevices)
        return fail(MCGP_E_NO_DEVICE, "device index out of range");
    *out = &g_ctx[device];
    return MCGP_OK;
}

void release_ctx(DeviceCtx &c)
{
    for (auto &sl : c.slot) {
        if (sl.dev) (void)hipFree(sl.dev);
        if (sl.host) (void)hipHostFree(sl.host);
        for (auto &rd : sl.reader)
            if (rd.done) (void)hipEventDestroy(rd.done);
        if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
        sl = DeviceCtx::Slot{};
    }
    if (c.d_hist) (void)hipFree(c.d_hist);
    if (c.d_grid) (void)hipFree(c.d_grid);
    if (c.d_order1) (void)hipFree(c.d_order1);
    if (c.d_fe_in) (void)hipFree(c.d_fe_in);
    if (c.d_fe_pen) (void)hipFree(c.d_fe_pen);
    if (c.d_fe_out) (void)hipFree(c.d_fe_out);
    if (c.d_norm53) (void)hipFree(c.d_norm53);
    c.d_hist = nullptr;
    c.d_grid = c.d_order1 = nullptr;
    c.d_fe_in = c.d_fe_out = c.d_norm53 = nullptr;
    c.d_fe_pen = nullptr;
    c.work.release();
    if (c.call_start) (void)hipEventDestroy(c.call_start);
    if (c.call_stop) (void)hipEventDestroy(c.call_stop);
    c.call_start = c.call_stop = nullptr;
    for (auto &t : c.timer) {
        if (t.start) (void)hipEventDestroy(t.start);
        if (t.stop) (void)hipEventDestroy(t.stop);
        if (t.d_ticket) (void)hipFree(t.d_ticket);
        t.retire.release();
        t = DeviceCtx::Timer{};
    }
    c.last_timer = -1;
}

// LDS per block a launch may use: what the device offers, or less under MCGP_LDS_PER_BLOCK (tests: a device / runtime
// that offers less LDS per block).
size_t lds_limit(size_t device_bytes)
{
    if (const char *e = std::getenv("MCGP_LDS_PER_BLOCK")) {
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v >= 16384 && v < device_bytes) return (size_t)v;
    }
    return device_bytes;
}

int init_ctx_body(int device, DeviceCtx &c)
{
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c.cu_count = prop.multiProcessorCount;
    c.lds_per_block = lds_limit(prop.sharedMemPerBlock);       // 160 KiB on gfx950
    for (auto &sl : c.slot) {
        HIP_TRY(hipMalloc(&sl.dev, mcgp::kRetireTabOffset + mcgp::kRetireTabMaxBytes));
        HIP_TRY(hipHostMalloc(&sl.host, mcgp::kRetireTabOffset + mcgp::kRetireTabMaxBytes));
        HIP_TRY(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
    }
    HIP_TRY(hipMalloc(&c.d_hist, sizeof(unsigned long long) * MCGP_MAX_CARS * MCGP_MAX_CARS));
    HIP_TRY(hipMalloc(&c.d_grid, MCGP_MAX_CARS));
    HIP_TRY(hipMalloc(&c.d_order1, MCGP_MAX_CARS));
    HIP_TRY(hipMalloc(&c.d_fe_in, sizeof(double) * 4 * MCGP_MAX_CARS));
    HIP_TRY(hipMalloc(&c.d_fe_pen, sizeof(int32_t) * MCGP_MAX_CARS));
    HIP_TRY(hipMalloc(&c.d_fe_out, sizeof(double) * MCGP_MAX_CARS * MCGP_MAX_CARS));
    HIP_TRY(hipMalloc(&c.d_norm53, sizeof(mcgp_normal53_table_bits)));
    HIP_TRY(hipMemcpy(c.d_norm53, mcgp_normal53_table_bits, sizeof(mcgp_normal53_table_bits), hipMemcpyHostToDevice));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::race_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_per_block));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::race_resume_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_per_block));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::race_trace_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_per_block));
    // (the register kernels raise their dynamic-LDS limit when they are selected: launch())
    return MCGP_OK;
}

// First use of a device: the CALLER HOLDS c.mu, so two threads making their first call on one
// device cannot both initialise it (nor one launch into buffers the other is still creating).
// A HIP failure part-way releases what was allocated; the next call starts from scratch.
int ensure_ctx_locked(int device, DeviceCtx &c)
{
    if (c.ready) return MCGP_OK;
    const int rc = init_ctx_body(device, c);
    if (rc != MCGP_OK) {
        release_ctx(c);
        return rc;
    }
    c.ready = true;
    return MCGP_OK;
}

int build_params(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                 mcgp::KParams *kp)
{
    const char *err = "";
    const int rc = mcgp::build_params(cfg, drv, grid_probs, n, kp, &err);
    return rc == MCGP_OK ? rc : fail(rc, err);
}

using KernelFn = void (*)(const mcgp::KParams *, uint64_t, uint64_t, uint32_t, uint32_t, unsigned long long *,
                          uint8_t *, const uint8_t *, uint32_t, uint32_t *, uint32_t *);

}  // namespace

// The register-resident instantiations are compiled one per translation unit (reg_inst.hip,
// -DMCGP_INST_N=<n>) so that the build runs in parallel; here they are only declared.
namespace mcgp {
#define X(N_)                                                                                                                   \
    extern template __global__ void race_kernel_reg<N_>(const KParams *, uint64_t, uint64_t, uint32_t, uint32_t,               \
                                                        unsigned long long *, uint8_t *, const uint8_t *, uint32_t, uint32_t *, \
                                                        uint32_t *);                                                           \
    extern template __global__ void race_kernel_reg<N_, kSmallBlockWaves>(const KParams *, uint64_t, uint64_t, uint32_t,       \
                                                                          uint32_t, unsigned long long *, uint8_t *,           \
                                                                          const uint8_t *, uint32_t, uint32_t *, uint32_t *);  \
    extern template __global__ void race_kernel_reg_wide<N_>(const KParams *, uint64_t, uint64_t, uint32_t, uint32_t,          \
                                                             unsigned long long *, uint8_t *, const uint8_t *, uint32_t,       \
                                                             uint32_t *, uint32_t *, const double *);                          \
    extern template __global__ void race_kernel_reg_batch<N_>(const KParams *, const BatchItem *, uint32_t, uint64_t,          \
                                                              unsigned long long *, uint32_t, uint32_t *, uint32_t *,      \
                                                              uint32_t);
MCGP_REG_SIZES(X)
#undef X
}  // namespace mcgp

namespace {

using BatchKernelFn = void (*)(const mcgp::KParams *, const mcgp::BatchItem *, uint32_t, uint64_t, unsigned long long *,
                               uint32_t, uint32_t *, uint32_t *, uint32_t);
using WideKernelFn = void (*)(const mcgp::KParams *, uint64_t, uint64_t, uint32_t, uint32_t, unsigned long long *,
                              uint8_t *, const uint8_t *, uint32_t, uint32_t *, uint32_t *, const double *);

// The register-resident instantiations of field size n, at entry n - 1: the default block shape, the small one
// (kSmallBlockWaves), the reference-width build (mcgp_config.deviates = MCGP_DEVIATES_53) and the batch kernel.
struct RegKernels {
    KernelFn reg, small;
    WideKernelFn wide;
    BatchKernelFn batch;
};
const RegKernels kRegKernels[] = {
#define X(N_) {&mcgp::race_kernel_reg<N_>, &mcgp::race_kernel_reg<N_, mcgp::kSmallBlockWaves>, \
               &mcgp::race_kernel_reg_wide<N_>, &mcgp::race_kernel_reg_batch<N_>},
    MCGP_REG_SIZES(X)
#undef X
};
static_assert(sizeof(kRegKernels) / sizeof(kRegKernels[0]) == MCGP_MAX_CARS, "one entry per field size 1..32");

// The instantiations of field size n, or null when it has none.
const RegKernels *reg_kernels(uint32_t n) { return n >= 1 && n <= MCGP_MAX_CARS ? &kRegKernels[n - 1] : nullptr; }

// MCGP_FORCE_GENERIC=1: every problem goes to the generic LDS kernel.
bool force_generic()
{
    const char *e = std::getenv("MCGP_FORCE_GENERIC");
    return e && e[0] == '1';
}

KernelFn select_kernel(const mcgp::KParams &kp, bool *is_reg)
{
    // (the generic kernel also takes lap times near zero and values near the ends of binary64: reg_kernel_serves)
    const RegKernels *rk = reg_kernels((uint32_t)kp.n);
    *is_reg = rk && !force_generic() && mcgp::reg_kernel_serves(kp);
    return *is_reg ? rk->reg : &mcgp::race_kernel;
}

// deviates = MCGP_DEVIATES_53 has the register kernel's code only: a problem that kernel does not take is refused.
int check_wide(const mcgp::KParams &kp)
{
    if (kp.wide && (!reg_kernels((uint32_t)kp.n) || !mcgp::reg_kernel_serves(kp)))
        return fail(MCGP_E_BAD_ARG, "deviates = MCGP_DEVIATES_53 serves the problems the register kernel takes "
                                    "(reg_kernel_serves: lap times clear of zero, overtake_delta >= 0)");
    return MCGP_OK;
}

// The generic-shaped kernels (resume, trace, strategy) have no 53-bit path; `what` is the subject of the message.
int check_deviates_32(const mcgp::KParams &kp, const char *what)
{
    if (kp.wide)
        return fail(MCGP_E_BAD_ARG, std::string("deviates: ") + what +
                                        " at MCGP_DEVIATES_32 only (the generic kernel has no 53-bit path)");
    return MCGP_OK;
}

// The prologue of the entry points that run from the grid or from a race state, in the order they call it: the source
// (exactly one of the two), the parameter block (`what`: the call, for check_deviates_32's message), the state as the
// kernels read it.  An entry point's own checks stand between these, where they always stood.
int check_source(const double *grid_probs, const mcgp_race_state *state)
{
    if (state && grid_probs) return fail(MCGP_E_BAD_ARG, "grid_probs must be NULL when a state is given");
    if (!state && !grid_probs) return fail(MCGP_E_BAD_ARG, "grid_probs is NULL (a run from the grid needs it)");
    return MCGP_OK;
}

int build_params_32(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n, const char *what,
                    mcgp::KParams *kp)
{
    const int rc = build_params(cfg, drv, grid_probs, n, kp);
    return rc == MCGP_OK ? check_deviates_32(*kp, what) : rc;
}

// *st: zero from the grid, else the packed state; sim_offset: the first simulation id for the kernels that take the ids
// from the state (the scenario kernels), 0 for those that take them from their own argument.
int pack_state(const mcgp_race_state *state, uint32_t n, int total_laps, uint64_t sim_offset, mcgp::ResumeState *st)
{
    std::memset(st, 0, sizeof(*st));
    if (!state) return MCGP_OK;
    const std::string err = mcgp::pack_race_state(*state, 0, n, total_laps, st);
    if (!err.empty()) return fail(MCGP_E_BAD_ARG, err);
    st->sim_offset = sim_offset;
    return MCGP_OK;
}

// Launch geometry: persistent blocks striding over batches of `block` simulations.  The register kernel's
// block size and LDS footprint are compile-time functions of the field size (RegGeo<N>, shared with the
// kernel); the number of blocks per CU follows from LDS and the kernel's register allocation.
void launch_geometry(const DeviceCtx &c, uint32_t n, bool is_reg, KernelFn kernel, uint64_t n_sims, uint32_t *grid,
                     uint32_t *block, uint32_t *lds, int reg_waves = 0 /* 0: the register kernel's default block shape */,
                     bool wide = false /* the reference-width build: its block also holds table rows (WideGeo) */, int total_laps = 0,
                     size_t lane_lds = 0 /* a generic-shaped kernel's own LDS bytes per lane behind the rows (mcgp_run_priors) */)
{
    // waves per CU the kernel's register allocation admits: 4 SIMDs x floor(512 / VGPRs, granule 8), at most 8 each
    int reg_cap = 8;
    {
        hipFuncAttributes attr;
        if (hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(kernel)) == hipSuccess && attr.numRegs > 0) {
            const int alloc = ((attr.numRegs + 7) / 8) * 8;
            int per_simd = 512 / alloc;
            if (per_simd > 8) per_simd = 8;
            if (per_simd < 1) per_simd = 1;
            reg_cap = 4 * per_simd;
        }
    }
    int waves = 1, blocks_per_cu = 1;
    size_t bytes = 0;
    if (is_reg) {
        waves = reg_waves ? reg_waves : mcgp::reg_block_waves((int)n);
        bytes = wide ? mcgp::wide_launch_lds_bytes((int)n, waves, total_laps)
                     : mcgp::shared_lds_bytes_reg((int)n) + (size_t)waves * 64 * mcgp::per_thread_lds_bytes_reg((int)n);
    } else {
        const size_t per_lane = mcgp::per_thread_lds_bytes((int)n) + lane_lds;
        const size_t per_wave = 64 * per_lane;
        waves = (int)((c.lds_per_block - mcgp::kSharedTableBytes) / per_wave);
        if (waves > 8) waves = 8;
        if (waves < 1) waves = 1;
        uint32_t threads = (uint32_t)waves * 64u;
        if (n_sims < threads) threads = (uint32_t)(((n_sims + 63) / 64) * 64);
        if (threads == 0) threads = 64;
        waves = (int)(threads / 64);
        bytes = mcgp::kSharedTableBytes + (size_t)threads * per_lane;
    }
    blocks_per_cu = (int)(c.lds_per_block / bytes);
    if (blocks_per_cu * waves > reg_cap) blocks_per_cu = reg_cap / waves;
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    const uint32_t threads = (uint32_t)waves * 64u;
    const uint64_t n_batches = (n_sims + threads - 1) / threads;
    uint64_t g = (uint64_t)c.cu_count * (uint64_t)blocks_per_cu;
    if (g > n_batches) g = n_batches;
    if (g < 1) g = 1;
    *grid = (uint32_t)g;
    *block = threads;
    *lds = (uint32_t)bytes;
}

// The launch shape of a generic-shaped kernel (resume, trace, strategy: the generic race kernel's block and LDS) for
// `n_sims` simulations; MCGP_E_HIP when its block needs more LDS than the device offers.  `name` is the kernel's, for
// the message.
int generic_geometry(const DeviceCtx &c, KernelFn kernel, const char *name, uint32_t n, uint64_t n_sims, uint32_t *grid,
                     uint32_t *block, uint32_t *lds, size_t lane_lds = 0)
{
    launch_geometry(c, n, false, kernel, n_sims, grid, block, lds, 0, false, 0, lane_lds);
    if (*lds > c.lds_per_block)
        return fail(MCGP_E_HIP, std::string("the ") + name + " kernel's block needs " + std::to_string(*lds) +
                                    " bytes of LDS, the device offers " + std::to_string(c.lds_per_block) + " per block");
    return MCGP_OK;
}

// Most simulations one kernel launch may take.  The per-block LDS histogram counts in uint32 and a cell
// can receive at most one count per simulation the block runs, so keeping the whole launch below 2^32
// simulations rules out a silent wrap; longer runs are split into several launches on the same stream
// (results do not depend on the split: draws are addressed by global simulation id).
uint64_t max_sims_per_launch()
{
    uint64_t cap = 0xFFFFFE00ull;                                       // < 2^32, a multiple of 512
    if (const char *e = std::getenv("MCGP_MAX_SIMS_PER_LAUNCH")) {      // tests exercise the split with a small cap
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v >= 1 && v < cap) cap = v;
    }
    return cap;
}

// Simulations per chunk of staged finishing orders (mcgp_run with orders_out, mcgp_run_championship, mcgp_run_from_state
// with orders_out): the staging holds kOrdersChunk x n bytes.
constexpr uint64_t kOrdersChunk = 1ull << 22;

// Staging budgets, so that device memory does not grow with n_sims: of mcgp_run_trace (one byte per lap, driver and
// simulation) and of the six scenario calls, mcgp_run_strategies, mcgp_run_penalties, mcgp_run_events, mcgp_run_paces,
// mcgp_run_combined and mcgp_run_weather (per scenario and simulation a byte per driver, and what the kind stages beside it:
// ScenarioKind::sim_bytes)
constexpr uint64_t kTraceStageBytes = 512ull << 20;
constexpr uint64_t kStrategyStageBytes = 256ull << 20;
// ... and of mcgp_run_gaps: one byte per recorded lap, row (n drivers + 1 lead + n_pairs pairs) and simulation.
constexpr uint64_t kGapsStageBytes = 512ull << 20;
// ... and of mcgp_run_pit_windows: five bytes per recorded lap, window and simulation (19 200 per simulation at 60 laps and
// 64 windows, so twice the gaps call's budget keeps a chunk above 50 000 simulations there).
constexpr uint64_t kWindowStageBytes = 1024ull << 20;
// ... and of mcgp_run_conditions: per simulation the finishing order (n bytes) and one u64 mask of the conditions met.
constexpr uint64_t kConditionsStageBytes = 256ull << 20;
// ... and of mcgp_run_stints: per driver and simulation one u64 record and one position byte.
constexpr uint64_t kStintsStageBytes = 256ull << 20;
// ... and of mcgp_run_moves: per lap and driver one byte, then per driver the grid slot and the classified position.
constexpr uint64_t kMovesStageBytes = 512ull << 20;

// Simulations in one chunk of such a staging: budget / bytes_per_sim, at most max_sims_per_launch(), in multiples of 256
// when it can.
uint64_t stage_chunk_sims(uint64_t budget, uint64_t bytes_per_sim)
{
    uint64_t chunk = std::min<uint64_t>(max_sims_per_launch(), std::max<uint64_t>(1, budget / bytes_per_sim));
    if (chunk >= 256) chunk = chunk / 256 * 256;
    return chunk;
}

// ... rounded down to whole rounds of the device under the generic-shaped `kernel` (every resident block one batch: a
// chunk of 5.5 rounds costs 6), and at most n_sims (run_analysis: the trace, gaps, conditions, stints and moves calls).
uint64_t stage_chunk_rounds(const DeviceCtx &c, uint32_t n, KernelFn kernel, uint64_t budget, uint64_t bytes_per_sim,
                            uint64_t n_sims)
{
    uint64_t chunk = stage_chunk_sims(budget, bytes_per_sim);
    uint32_t g = 0, b = 0, l = 0;
    launch_geometry(c, n, false, kernel, chunk, &g, &b, &l);
    const uint64_t round = (uint64_t)g * b;
    if (chunk >= round) chunk = chunk / round * round;
    return std::min<uint64_t>(chunk, n_sims);
}

// Front-end inputs of one call, already on the device (c.d_fe_in / c.d_fe_pen), or null.
struct FrontEnd {
    bool on = false;
};

// The timing events and work counter of `stream` (its most recent call); the least recently used entry is recycled.
int claim_timer(DeviceCtx &c, hipStream_t stream, int *out)
{
    int ti = -1;
    for (int i = 0; i < kStreamTimers; ++i)
        if (c.timer[i].used && c.timer[i].stream == stream) { ti = i; break; }
    if (ti < 0) {
        ti = 0;
        for (int i = 0; i < kStreamTimers; ++i) {
            if (!c.timer[i].used) { ti = i; break; }
            if (c.timer[i].seq < c.timer[ti].seq) ti = i;
        }
        if (!c.timer[ti].d_ticket) {
            // events and counter are created into locals and committed together: a failure part-way leaves the entry
            // empty (not an entry with events and a NULL counter for the next launch to hand to the kernel)
            hipEvent_t e0 = nullptr, e1 = nullptr;
            uint32_t *tk = nullptr;
            hipError_t err = hipEventCreate(&e0);
            if (err == hipSuccess) err = hipEventCreate(&e1);
            if (err == hipSuccess) err = hipMalloc(&tk, sizeof(uint32_t));
            if (err != hipSuccess) {
                if (e0) (void)hipEventDestroy(e0);
                if (e1) (void)hipEventDestroy(e1);
                return fail(err == hipErrorOutOfMemory ? MCGP_E_NOMEM : MCGP_E_HIP,
                            std::string("stream timer / work counter: ") + hipGetErrorString(err));
            }
            c.timer[ti].start = e0;
            c.timer[ti].stop = e1;
            c.timer[ti].d_ticket = tk;
        } else if (c.timer[ti].used) {
            // recycled from another stream: its last launch may still be claiming work from the entry's counter
            HIP_TRY(hipEventSynchronize(c.timer[ti].stop));
        }
        c.timer[ti].stream = stream;
        c.timer[ti].used = true;
    }
    *out = ti;
    return MCGP_OK;
}

// The pair of timing events of a call that runs several kernels (on_device): recorded on the null stream around
// everything the call runs, so that mcgp_last_kernel_ms afterwards gives the whole call.
int ensure_call_events(DeviceCtx &c)
{
    if (c.call_start) return MCGP_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    if (err != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        return fail(MCGP_E_HIP, std::string("batch timing events: ") + hipGetErrorString(err));
    }
    c.call_start = e0;
    c.call_stop = e1;
    return MCGP_OK;
}

// The launch that mcgp_last_launch_info and mcgp_last_kernel_name report: its shape and its kernel's name (a printf
// format and its arguments).
__attribute__((format(printf, 5, 6))) void note_launch(DeviceCtx &c, uint32_t grid, uint32_t block, uint32_t lds,
                                                       const char *name, ...)
{
    c.last_grid = grid;
    c.last_block = block;
    c.last_lds = lds;
    va_list args;
    va_start(args, name);
    std::vsnprintf(c.last_kernel, sizeof(c.last_kernel), name, args);
    va_end(args);
}

int launch(DeviceCtx &c, const mcgp::KParams &kp, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
           hipStream_t stream, unsigned long long *d_hist, uint8_t *d_orders, const uint8_t *d_fixed_grid,
           const FrontEnd &fe = FrontEnd())
{
    if (n_sims == 0) return MCGP_OK;
    bool is_reg = false;
    KernelFn kernel = select_kernel(kp, &is_reg);
    // the reference-width build (mcgp_config.deviates = MCGP_DEVIATES_53): the register kernel's geometry, its own code
    WideKernelFn wide = nullptr;
    if (kp.wide) {
        const int rc = check_wide(kp);
        if (rc != MCGP_OK) return rc;
        wide = reg_kernels((uint32_t)kp.n)->wide;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(wide), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)c.lds_per_block));
        is_reg = true;
        kernel = nullptr;
    }
    DeviceCtx::Slot *sl = nullptr;
    if (!fe.on)           // a block whose matrix is written by the device front end is never shared
        for (auto &cand : c.slot)
            if (cand.used && cand.shareable && std::memcmp(cand.host, &kp, sizeof(kp)) == 0) { sl = &cand; break; }
    if (!sl) {
        sl = &c.slot[c.next_slot];
        c.next_slot = (c.next_slot + 1) % kParamSlots;
        if (sl->used)                                           // every stream that read it has finished
            for (auto &rd : sl->reader)
                if (rd.live) {
                    HIP_TRY(hipEventSynchronize(rd.done));
                    rd.live = false;
                }
        std::memcpy(sl->host, &kp, sizeof(kp));
        sl->used = true;
        sl->shareable = !fe.on;
        // the register kernels' retirement table, behind the block (built for every block: which kernel serves a
        // re-used block is decided per launch)
        mcgp::build_retire_table(kp, kp.wide != 0, reinterpret_cast<unsigned char *>(sl->host) + mcgp::kRetireTabOffset);
        const size_t upload = mcgp::kRetireTabOffset + mcgp::retire_table_bytes(kp.n, kp.total_laps, kp.wide != 0);
        HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, upload, hipMemcpyHostToDevice, stream));
        if (fe.on) {
            // the n x n matrix goes from the front-end kernel straight into the block's grid_probs slot, on
            // the launch stream, between the upload and the race kernel (the slot is marked not shareable:
            // its pinned host copy, still being read by the asynchronous upload, no longer describes it)
            hipLaunchKernelGGL(grid_probs_kernel, dim3(1), dim3(mcgp::kMaxCars), 0, stream, c.d_fe_in, c.d_fe_pen,
                               (int)kp.n, sl->dev->grid_probs);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(sl->uploaded, stream));
        sl->upload_stream = stream;
    } else if (sl->upload_stream != stream) {
        // cached block uploaded on another stream: order this stream behind that upload
        HIP_TRY(hipStreamWaitEvent(stream, sl->uploaded, 0));
    }
    int ti = -1;
    {
        const int rc = claim_timer(c, stream, &ti);
        if (rc != MCGP_OK) return rc;
    }
    c.timer[ti].seq = ++c.timer_seq;
    if (!c.timer[ti].d_ticket) return fail(MCGP_E_HIP, "no work counter for this stream");
    HIP_TRY(hipEventRecord(c.timer[ti].start, stream));
    const uint64_t cap = max_sims_per_launch();
    uint32_t grid = 0, block = 0, lds = 0;
    // The register kernel's default block fills the CU's LDS to the last half kilobyte at 20 cars (RegGeo).  A device or a
    // runtime that offers less per block gets the same kernel in blocks of kSmallBlockWaves waves -- less than half the
    // footprint, about 15 % slower --: chosen up front when the device reports less LDS than the block needs, and once more,
    // with a fresh launch, when the launch itself is refused for its resources.  The shape in use shows in
    // mcgp_last_launch_info (block_threads) and mcgp_last_kernel_name.
    bool small_shape = false;
    auto resource_error = [](hipError_t e) {
        return e == hipErrorOutOfMemory || e == hipErrorInvalidValue || e == hipErrorLaunchOutOfResources ||
               e == hipErrorInvalidConfiguration;
    };
    for (uint64_t done = 0; done < n_sims; done += cap) {
        const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
        for (;;) {
            // (small_shape is only ever set for the register kernel, whose field size has an entry)
            const KernelFn k = small_shape ? reg_kernels((uint32_t)kp.n)->small : kernel;
            launch_geometry(c, (uint32_t)kp.n, is_reg, wide ? reinterpret_cast<KernelFn>(wide) : k, m, &grid, &block, &lds,
                            wide ? mcgp::wide_block_waves(kp.n) : small_shape ? mcgp::kSmallBlockWaves : 0, wide != nullptr,
                            kp.total_laps);
            const bool may_shrink = is_reg && !wide && !small_shape;
            if (may_shrink && lds > c.lds_per_block) {              // the device offers less than the default block needs
                small_shape = true;
                continue;
            }
            if (lds > c.lds_per_block)
                return fail(MCGP_E_HIP, "the kernel's smallest block needs " + std::to_string(lds) + " bytes of LDS, the device offers " +
                                            std::to_string(c.lds_per_block) + " per block");
            if (is_reg && !wide) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    if (may_shrink && resource_error(e)) { small_shape = true; continue; }
                    return fail(MCGP_E_HIP, std::string("hipFuncSetAttribute(dynamic LDS): ") + hipGetErrorString(e));
                }
            }
            // units of work: the register kernel's waves claim chunks of 64 simulations from the stream's counter, a block
            // of the generic kernel takes batches of `block` by its index (both < 2^32 because m < 2^32)
            const uint64_t unit = is_reg ? 64u : block;
            const uint64_t n_batches = (m + unit - 1) / unit;
            DevBuf &retire = c.timer[ti].retire;
            if (is_reg) {
                HIP_TRY(hipMemsetAsync(c.timer[ti].d_ticket, 0, sizeof(uint32_t), stream));
                // the lanes' retirement lists: scratch of the launch, (n + 1) words per lane, kept per stream and grown on
                // demand (a launch of this stream that still uses the old buffer has been enqueued before the free, which
                // the runtime orders behind it)
                const size_t want = mcgp::reg_retire_ws_bytes(kp.n, (size_t)grid * block);
                if (want > retire.bytes && retire.p) HIP_TRY(hipStreamSynchronize(stream));
                const int rc = retire.reserve(want);
                if (rc != MCGP_OK) return rc;
            }
            if (wide)
                hipLaunchKernelGGL(wide, dim3(grid), dim3(block), lds, stream, sl->dev, m, sim_offset + done,
                                   (uint32_t)seed, (uint32_t)(seed >> 32), d_hist,
                                   d_orders ? d_orders + (size_t)done * (size_t)kp.n : nullptr, d_fixed_grid,
                                   (uint32_t)n_batches, c.timer[ti].d_ticket, retire.at<uint32_t>(), c.d_norm53);
            else
                hipLaunchKernelGGL(k, dim3(grid), dim3(block), lds, stream, sl->dev, m, sim_offset + done,
                                   (uint32_t)seed, (uint32_t)(seed >> 32), d_hist,
                                   d_orders ? d_orders + (size_t)done * (size_t)kp.n : nullptr, d_fixed_grid,
                                   (uint32_t)n_batches, c.timer[ti].d_ticket, retire.at<uint32_t>());
            const hipError_t e = hipGetLastError();
            if (e == hipSuccess) break;
            if (may_shrink && resource_error(e)) {                  // refused for its resources: once more, small blocks
                small_shape = true;
                continue;
            }
            return fail(e == hipErrorOutOfMemory ? MCGP_E_NOMEM : MCGP_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
        }
    }
    HIP_TRY(hipEventRecord(c.timer[ti].stop, stream));
    c.last_timer = ti;
    {
        // completion event of (this block, this stream)
        DeviceCtx::Slot::Reader *rd = nullptr, *spare = nullptr;
        for (auto &r : sl->reader) {
            if (r.live && r.stream == stream) { rd = &r; break; }
            // an entry whose launch has completed is free again (it used to stay "live" until the block was evicted,
            // so that the ninth stream on a long-lived block blocked the host on entry 0 -- the most recent launch)
            if (r.live && hipEventQuery(r.done) == hipSuccess) r.live = false;
            if (!r.live && !spare) spare = &r;
        }
        if (!rd) {
            if (!spare) {                               // more streams IN FLIGHT than entries: wait for the oldest launch
                spare = &sl->reader[0];
                for (auto &r : sl->reader)
                    if (r.seq < spare->seq) spare = &r;
                HIP_TRY(hipEventSynchronize(spare->done));
            }
            rd = spare;
            if (!rd->done) HIP_TRY(hipEventCreateWithFlags(&rd->done, hipEventDisableTiming));
            rd->stream = stream;
            rd->live = true;
        }
        rd->seq = c.timer_seq;
        HIP_TRY(hipEventRecord(rd->done, stream));
    }
    if (wide) note_launch(c, grid, block, lds, "mcgp::race_kernel_reg_wide<%d>", kp.n);
    else if (is_reg && small_shape) note_launch(c, grid, block, lds, "mcgp::race_kernel_reg<%d, %d>", kp.n, mcgp::kSmallBlockWaves);
    else if (is_reg) note_launch(c, grid, block, lds, "mcgp::race_kernel_reg<%d>", kp.n);
    else note_launch(c, grid, block, lds, "mcgp::race_kernel");
    return MCGP_OK;
}

// One segment of a call's counts: a caller's buffer (NULL: not wanted) and its cells.  A call lists its segments once,
// in the order they have on the device, for Layout::counts and for Counts::add_to.
struct CountSeg {
    uint64_t *dst;
    size_t cells;
};

// One call's regions in the workspace, each rounded up to 256 bytes.  add(size) only reserves and returns the offset.
// add(&pointer, count, source) declares a region of `count` items together with the device pointer that is to address
// it and, for an input, the host array it is filled from; counts(segments) declares the call's counts, one block of
// u64 cells.  commit() then reserves the workspace, points every declared pointer at its region, uploads the sources
// and zeroes the counts (on the null stream, like everything these calls do).
struct Layout {
    size_t bytes = 0;
    size_t add(size_t region)
    {
        const size_t at = bytes;
        bytes += (region + 255) / 256 * 256;
        return at;
    }
    template <class T, class U = T> void add(T **at, size_t count, const U *src = nullptr)
    {
        regions.push_back({add(sizeof(T) * count), (void **)at, src, src ? sizeof(T) * count : 0});
    }
    void counts(const std::vector<CountSeg> &segs)
    {
        for (const CountSeg &s : segs) {
            seg_at.push_back(count_cells);
            count_cells += s.cells;
        }
        o_counts = add(count_cells * 8);
    }
    int commit(DevBuf &buf)
    {
        const int rc = buf.reserve(bytes);
        if (rc != MCGP_OK) return rc;
        for (const Region &g : regions) {
            *g.at = buf.at(g.offset);
            if (g.bytes) HIP_TRY(hipMemcpy(*g.at, g.src, g.bytes, hipMemcpyHostToDevice));
        }
        d_counts = buf.at<unsigned long long>(o_counts);
        if (count_cells) HIP_TRY(hipMemsetAsync(d_counts, 0, count_cells * 8, nullptr));
        return MCGP_OK;
    }
    // segment i of the counts on the device (after commit)
    unsigned long long *count(size_t i) const { return d_counts + seg_at[i]; }

    struct Region {
        size_t offset;
        void **at;
        const void *src;
        size_t bytes;                       // to upload (0: no source)
    };
    std::vector<Region> regions;
    std::vector<size_t> seg_at;
    size_t count_cells = 0, o_counts = 0;
    unsigned long long *d_counts = nullptr;
};

// The counts of one call: downloaded in one piece while the call holds its context, then added into the caller's
// buffers once the whole call has returned MCGP_OK.  No entry point adds into a caller's buffer any other way, so a call
// that fails leaves them untouched (and a retry counts nothing twice).
struct Counts {
    using Seg = CountSeg;
    std::vector<unsigned long long> v;
    int download(const void *d_src, size_t cells)
    {
        v.resize(cells);
        HIP_TRY(hipMemcpy(v.data(), d_src, cells * 8, hipMemcpyDeviceToHost));
        return MCGP_OK;
    }
    int download(const Layout &ws) { return download(ws.d_counts, ws.count_cells); }
    void add_to(const std::vector<Seg> &segs) const     // segs: in the order of the counts on the device
    {
        const unsigned long long *src = v.data();
        for (const Seg &s : segs) {
            if (s.dst)
                for (size_t i = 0; i < s.cells; ++i) s.dst[i] += src[i];
            src += s.cells;
        }
    }
};

// One call on `device`: looks its context up, holds the context's lock for the whole call, initialises it on first use,
// makes the device current and runs body(context).  timed: a call of several kernels, bracketed on the null stream by
// the call's own pair of events, so that mcgp_last_kernel_ms afterwards gives everything it ran; once the start is
// recorded the stop is recorded too, whatever the body returns, so that no start is left paired with an older stop.
template <class Body>
int on_device(int32_t device, bool timed, Body &&body)
{
    DeviceCtx *c = nullptr;
    int rc = find_ctx(device, &c);
    if (rc != MCGP_OK) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    rc = ensure_ctx_locked(device, *c);
    if (rc != MCGP_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!timed) return body(*c);
    rc = ensure_call_events(*c);
    if (rc != MCGP_OK) return rc;
    HIP_TRY(hipEventRecord(c->call_start, nullptr));
    rc = body(*c);
    const hipError_t e = hipEventRecord(c->call_stop, nullptr);
    c->last_timer = e == hipSuccess ? kCallTimer : -1;        // (a pair without its stop is not reported)
    if (rc == MCGP_OK && e != hipSuccess) return fail(MCGP_E_HIP, std::string("call timing event: ") + hipGetErrorString(e));
    return rc;
}

// The loop of the calls that stage per-simulation results on the device and count them there: n_sims simulations in
// chunks of `chunk`, each chunk in the launch shape of the generic-shaped kernel `geo_fn` (`geo_name`: its name in the LDS
// message) -- the blocks the device holds at once shared out over `rows` grid rows, 1 for a call without scenarios --
// handed to body(done, m, gx, block, lds, n_batches): simulations done .. done + m - 1 of the call in a launch of (gx,
// rows) blocks, each striding over the chunk's n_batches batches of `block` simulations.  The body launches the race
// and its counting kernels, before the next chunk overwrites the staging.  Afterwards the first (fullest) chunk's shape
// is what mcgp_last_launch_info reports, under `kernel_name`, and the counts laid out in `ws` are downloaded.  lane_lds:
// the kernel's own LDS bytes per lane behind the generic rows (launch_geometry).
template <class Body>
int staged_run(DeviceCtx &c, KernelFn geo_fn, const char *geo_name, const char *kernel_name, uint32_t n, uint32_t rows,
               uint64_t n_sims, uint64_t chunk, const Layout &ws, Counts &counts, Body &&body, size_t lane_lds = 0)
{
    uint32_t grid0 = 0, block0 = 0, lds0 = 0;
    for (uint64_t done = 0; done < n_sims; done += chunk) {
        const uint64_t m = (n_sims - done) < chunk ? (n_sims - done) : chunk;
        uint32_t grid = 0, block = 0, lds = 0;
        int r = generic_geometry(c, geo_fn, geo_name, n, m * rows, &grid, &block, &lds, lane_lds);
        if (r != MCGP_OK) return r;
        const uint64_t n_batches = (m + block - 1) / block;
        const uint32_t gx = (uint32_t)std::min<uint64_t>(n_batches, (grid + rows - 1) / rows);
        if (done == 0) { grid0 = gx * rows; block0 = block; lds0 = lds; }
        r = body(done, m, gx, block, lds, (uint32_t)n_batches);
        if (r != MCGP_OK) return r;
    }
    note_launch(c, grid0, block0, lds0, "%s", kernel_name);
    return counts.download(ws);
}

// One chunk of a scenario call as its kernels are launched: (gx, S) blocks of `block` threads over simulations
// first_sim .. first_sim + m - 1, the shared inputs and outputs on the device.
struct ScenarioChunk {
    uint32_t gx, S, block, lds, n_batches;
    uint64_t m, first_sim, seed;
    const mcgp::KParams *kp;
    const mcgp::ResumeState *st;
    const mcgp::StrategyScenario *sc;
    const mcgp::StopLap *sl;
    unsigned long long *hist;
    uint8_t *stage;                         // [S][m][n] bytes: every driver's finishing position
    // the tables of the kind's rule sets, and what they stage beside the bytes; NULL where the kind has none or the
    // output is not wanted (ScenarioKind::regions lays them out)
    const mcgp::PenaltyScenario *pn;
    const mcgp::PenaltyLap *nl;
    const uint8_t *el;                      // (with weather: the laps' condition bytes)
    const mcgp::PaceScenario *ps;
    const mcgp::PaceLap *pl;
    const double *sec;                      // (with weather: the table of wrong-tyre seconds)
    uint32_t *evs;                          // [S][m] packed event counts
    uint16_t *car;                          // [S][m][n] laps carried (with weather: laps on the wrong tyres; with grid
                                            // edits: start slots)
    const mcgp::GridScenario *gr;           // with grid edits: the edit table, which the kernel reads through `pens`
    // with priors: the item table, which the kernel reads through `pens`; [S][m][n] bins of the drawn offsets, which it
    // writes through `carried`; [S][m][n] offsets (NULL: not wanted), which it writes through `ev_stage`
    const mcgp::PriorScenario *pr;
    uint8_t *bins;
    float *offs;
};

// Grid width of a counting kernel over m simulations in blocks of `block` threads: the tiles, but no more blocks than
// the device holds at once shared out over the grid's `rows` rows (and layers), and at least one.
uint32_t count_grid_x(uint64_t m, uint32_t block, uint64_t grid_cap, uint64_t rows)
{
    const uint64_t tiles = (m + block - 1) / block;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, grid_cap / rows));
}

// The counting kernels of the rule sets over a chunk's staging, one grid row per scenario; mcgp_run_combined runs all
// three, each on the staging in its own layout.  delta and the kind's own segment are NULL for what is not wanted.
void count_penalties(const ScenarioChunk &l, uint32_t n, uint64_t grid_cap, unsigned long long *delta, unsigned long long *fate)
{
    hipLaunchKernelGGL(mcgp::penalties_count, dim3(count_grid_x(l.m, mcgp::kPenaltyCountBlock, grid_cap, l.S), l.S),
                       dim3(mcgp::kPenaltyCountBlock), 0, nullptr, l.stage, l.m, n, delta, fate);
}

void count_events(const ScenarioChunk &l, uint32_t n, uint32_t L, uint64_t grid_cap, unsigned long long *delta,
                  unsigned long long *events)
{
    hipLaunchKernelGGL(mcgp::events_count, dim3(count_grid_x(l.m, mcgp::kEventsCountBlock, grid_cap, l.S), l.S),
                       dim3(mcgp::kEventsCountBlock), 0, nullptr, l.stage, l.evs, l.m, n, L, delta, events);
}

// grid layers: the deltas (a layer that returns at once when delta is NULL), then (carried wanted) one per driver
void count_paces(const ScenarioChunk &l, uint32_t n, uint32_t L, uint64_t grid_cap, unsigned long long *delta,
                 unsigned long long *carried)
{
    const uint32_t gz = carried ? 1u + n : 1u;
    hipLaunchKernelGGL(mcgp::paces_count, dim3(count_grid_x(l.m, mcgp::kPacesCountBlock, grid_cap, (uint64_t)l.S * gz), l.S, gz),
                       dim3(mcgp::kPacesCountBlock), 0, nullptr, l.stage, l.car, l.ps, l.m, n, L, delta, carried);
}

// One item table of a scenario call beside the plans, one count per scenario: the arguments, their names and the check of
// the counts before anything is packed.
struct ScenarioTable {
    const char *count_name, *items_name;
    const uint32_t *item_count;
    const void *items;
    std::function<std::string(uint64_t *n_items)> check_counts;
};

// One count segment of a scenario call behind hist and delta: the caller's buffer (NULL: not wanted), its cells, a
// fix-up on the host (empty: none).
struct ScenarioOutput {
    uint64_t *out;
    std::function<size_t(size_t S, size_t n, size_t L)> cells;
    std::function<void(unsigned long long *extra, size_t rows, uint64_t n_sims)> fix_up;
};

// What mcgp_run_strategies, mcgp_run_penalties, mcgp_run_events, mcgp_run_paces, mcgp_run_combined, mcgp_run_weather,
// mcgp_run_grids and mcgp_run_priors each have of their own; run_scenarios has the rest.
struct ScenarioKind {
    const char *what;                       // the call in check_deviates_32's message
    // generic_geometry's and note_launch's name of the race kernel.  These are the documented names of the calls
    // (include/mcgp.h: mcgp_last_kernel_name), not of symbols: every kind runs an instantiation of race_scenario_kernel
    const char *geo_name, *kernel_name;
    uint32_t rules;                         // the kind's rule sets (mcgp::kRule*): the instantiation that runs
    std::vector<ScenarioTable> tables;                                   // the kind's own input tables, checked in this order
    std::function<std::string(int first_lap, bool resumed)> pack;        // their items, behind pack_scenarios
    size_t sim_bytes = 0;                                                // staged per (scenario, simulation)
    uint8_t pos_mask = 0xFF;                                             // the position in a staged byte
    // its regions of the workspace: the tables and staging of its rule sets, into the chunk's pointers
    std::function<void(Layout &, ScenarioChunk &, uint64_t chunk)> regions;
    // launches the counting kernels (run when delta or one of the kind's outputs is wanted): delta and extra[i], the
    // device segment of outputs[i], are NULL for what is not wanted
    std::function<void(const ScenarioChunk &, uint64_t grid_cap, unsigned long long *delta, unsigned long long *const *extra)>
        count;
    std::vector<ScenarioOutput> outputs;                                 // the kind's own count segments
    size_t lane_lds = 0;                                                 // its lanes' own LDS bytes behind the generic rows
    // what it reads back per chunk beside the counts (simulations done .. done + m - 1 of the call are staged), into
    // memory of its own, and hands to the caller once everything has run; empty: nothing
    std::function<int(const ScenarioChunk &, uint64_t done)> read_back;
    std::function<void()> hand_over;
};

int32_t run_scenarios(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                      uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                      uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                      uint64_t *delta_out, uint8_t *orders_out, const ScenarioKind &k)
{
    // ---- every argument is checked before any device is looked up
    if (!hist_out) return fail(MCGP_E_BAD_ARG, "hist_out is NULL");
    if (!plan_count) return fail(MCGP_E_BAD_ARG, "plan_count is NULL");
    for (const ScenarioTable &t : k.tables)
        if (!t.item_count) return fail(MCGP_E_BAD_ARG, std::string(t.count_name) + " is NULL");
    if (n_scenarios < 1 || n_scenarios > mcgp::kMaxStrategyScenarios)
        return fail(MCGP_E_BAD_ARG, "n_scenarios must be in [1, 64]");
    uint64_t n_plans = 0;
    std::vector<uint64_t> n_items(k.tables.size(), 0);
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (plan_count[si] > mcgp::kMaxCars)
            return fail(MCGP_E_BAD_ARG, "scenario " + std::to_string(si) + ": plan_count must be in [0, 32]");
        n_plans += plan_count[si];
    }
    for (size_t ti = 0; ti < k.tables.size(); ++ti) {
        const std::string err = k.tables[ti].check_counts(&n_items[ti]);
        if (!err.empty()) return fail(MCGP_E_BAD_ARG, err);
    }
    if (n_plans && !plans) return fail(MCGP_E_BAD_ARG, "plans is NULL");
    for (size_t ti = 0; ti < k.tables.size(); ++ti)
        if (n_items[ti] && !k.tables[ti].items) return fail(MCGP_E_BAD_ARG, std::string(k.tables[ti].items_name) + " is NULL");
    int rc = check_source(grid_probs, state);
    if (rc != MCGP_OK) return rc;
    std::vector<mcgp::KParams> kps(1);
    mcgp::KParams &kp = kps[0];
    rc = build_params_32(cfg, drv, grid_probs, n, k.what, &kp);
    if (rc != MCGP_OK) return rc;
    const int L = cfg->total_laps;
    mcgp::ResumeState st;
    rc = pack_state(state, n, L, sim_offset, &st);
    if (rc != MCGP_OK) return rc;
    const int first_lap = state ? st.lap + 1 : 2;
    std::vector<mcgp::StrategyScenario> scen;
    std::vector<mcgp::StopLap> stop_laps;
    {
        std::string err = mcgp::pack_scenarios(n_scenarios, plan_count, plans, n, L, first_lap, state != nullptr, &scen,
                                               &stop_laps);
        if (err.empty() && k.pack) err = k.pack(first_lap, state != nullptr);
        if (!err.empty()) return fail(MCGP_E_BAD_ARG, err);
    }
    if (n_sims == 0) return MCGP_OK;
    const uint32_t S = n_scenarios;
    const size_t w = 2 * (size_t)n - 1;
    const size_t c_hist = (size_t)S * n * n, c_delta = (size_t)S * n * w;
    // hist [S][n][n] | delta [S][n][2n - 1] | the kind's own counts
    std::vector<Counts::Seg> segs = {{hist_out, c_hist}, {delta_out, c_delta}};
    bool want_extra = false;
    for (const ScenarioOutput &o : k.outputs) {
        segs.push_back({o.out, o.cells(S, n, (size_t)L)});
        want_extra |= o.out != nullptr;
    }
    Counts counts;
    std::vector<uint8_t> orders;            // collected on the host, handed over only once everything has run
    rc = on_device(device, true, [&](DeviceCtx &c) -> int {
        const uint64_t chunk = std::min<uint64_t>(stage_chunk_sims(kStrategyStageBytes, (uint64_t)S * k.sim_bytes), n_sims);
        const size_t stage_bytes = (size_t)S * chunk * n;
        // workspace: staged positions of a chunk | parameter block | state | scenarios | stop laps | the kind's regions |
        // the counts
        ScenarioChunk l = {};
        Layout ws;
        ws.add(&l.stage, stage_bytes);
        ws.add(&l.kp, 1, &kp);
        ws.add(&l.st, 1, &st);
        ws.add(&l.sc, S, scen.data());
        ws.add(&l.sl, stop_laps.size(), stop_laps.data());
        if (k.regions) k.regions(ws, l, chunk);
        ws.counts(segs);
        const int r = ws.commit(c.work);
        if (r != MCGP_OK) return r;
        l.hist = ws.count(0);
        l.S = S;
        l.seed = seed;
        std::vector<uint8_t> pos_back;
        if (orders_out) {
            pos_back.resize(stage_bytes);
            orders.resize((size_t)S * n_sims * n);
        }
        const uint64_t grid_cap = (uint64_t)c.cu_count * 8;
        const bool count_delta = delta_out && S > 1;
        // the instantiation that runs is also the one whose register count shapes the launch
        const mcgp::ScenarioKernel kernel = mcgp::scenario_kernel(k.rules, state != nullptr);
        return staged_run(c, reinterpret_cast<KernelFn>(kernel), k.geo_name, k.kernel_name, n, S, n_sims, chunk, ws, counts,
                          [&](uint64_t done, uint64_t m, uint32_t gx, uint32_t block, uint32_t lds, uint32_t n_batches) -> int {
            l.gx = gx, l.block = block, l.lds = lds, l.n_batches = n_batches, l.m = m, l.first_sim = sim_offset + done;
            const mcgp::PenaltyScenario *pens = l.gr   ? reinterpret_cast<const mcgp::PenaltyScenario *>(l.gr)
                                                : l.pr ? reinterpret_cast<const mcgp::PenaltyScenario *>(l.pr) : l.pn;
            uint32_t *evs = l.pr ? reinterpret_cast<uint32_t *>(l.offs) : l.evs;
            uint16_t *car = l.pr ? reinterpret_cast<uint16_t *>(l.bins) : l.car;
            hipLaunchKernelGGL(kernel, dim3(l.gx, l.S), dim3(l.block), l.lds, nullptr, l.kp, l.st, l.sc, l.sl, pens, l.nl, l.el,
                               l.ps, l.pl, l.sec, l.m, l.first_sim, (uint32_t)l.seed, (uint32_t)(l.seed >> 32), l.hist, l.stage,
                               evs, car, l.n_batches);
            HIP_TRY(hipGetLastError());
            if (count_delta || want_extra) {
                std::vector<unsigned long long *> extra;
                for (size_t oi = 0; oi < k.outputs.size(); ++oi) extra.push_back(k.outputs[oi].out ? ws.count(2 + oi) : nullptr);
                k.count(l, grid_cap, count_delta ? ws.count(1) : nullptr, extra.data());
                HIP_TRY(hipGetLastError());
            }
            if (orders_out) {
                HIP_TRY(hipMemcpy(pos_back.data(), l.stage, (size_t)S * m * n, hipMemcpyDeviceToHost));
                for (uint32_t si = 0; si < S; ++si)
                    for (uint64_t i = 0; i < m; ++i) {
                        const uint8_t *pos = pos_back.data() + ((size_t)si * m + i) * n;
                        uint8_t *ord = orders.data() + ((size_t)si * n_sims + done + i) * n;
                        for (uint32_t d = 0; d < n; ++d) ord[pos[d] & k.pos_mask] = (uint8_t)d;
                    }
            }
            return k.read_back ? k.read_back(l, done) : MCGP_OK;
        }, k.lane_lds);
    });
    if (rc != MCGP_OK) return rc;
    unsigned long long *b = counts.v.data() + c_hist;
    if (delta_out) {
        // the centre bin (no change) of every (scenario, driver) is what the other bins leave of n_sims
        for (size_t row = 0; row < (size_t)S * n; ++row) {
            unsigned long long rest = 0;
            for (size_t j = 0; j < w; ++j) rest += j == n - 1 ? 0ull : b[row * w + j];
            b[row * w + n - 1] = n_sims - rest;
        }
    }
    {
        unsigned long long *x = b + c_delta;
        for (const ScenarioOutput &o : k.outputs) {
            if (o.out && o.fix_up) o.fix_up(x, (size_t)S * n, n_sims);
            x += o.cells(S, n, (size_t)L);
        }
    }
    counts.add_to(segs);
    if (orders_out) std::memcpy(orders_out, orders.data(), orders.size());
    if (k.hand_over) k.hand_over();
    return MCGP_OK;
}

// fate [S][n][4]; column 0 (no SERVE_AT_STOP penalty) is, like delta's centre bin, what the others leave of n_sims
ScenarioOutput fate_output(uint64_t *fate_out)
{
    return {fate_out, [](size_t S, size_t n, size_t) { return S * n * 4; },
            [](unsigned long long *f, size_t rows, uint64_t n_sims) {
                for (size_t row = 0; row < rows; ++row) f[row * 4] = n_sims - (f[row * 4 + 1] + f[row * 4 + 2] + f[row * 4 + 3]);
            }};
}

// events [S][3][L + 1]
ScenarioOutput events_output(uint64_t *events_out)
{
    return {events_out, [](size_t S, size_t, size_t L) { return S * 3 * (L + 1); }, nullptr};
}

// carried [S][n][L + 1]; column 0 is, like delta's centre bin, what the others leave of n_sims: all of it for a driver
// without an UNTIL_STOP offset
ScenarioOutput carried_output(uint64_t *carried_out, const mcgp_config *cfg)
{
    return {carried_out, [](size_t S, size_t n, size_t L) { return S * n * (L + 1); },
            [cfg](unsigned long long *c, size_t rows, uint64_t n_sims) {      // (cfg has been checked by then)
                const size_t w = (size_t)cfg->total_laps + 1;
                for (size_t row = 0; row < rows; ++row) {
                    unsigned long long rest = 0;
                    for (size_t j = 1; j < w; ++j) rest += c[row * w + j];
                    c[row * w] = n_sims - rest;
                }
            }};
}

// One chunk of an analysis call as its kernels are launched: `grid` blocks of `block` threads over simulations first_sim
// .. first_sim + m - 1, staged in rows of `stride` items, and the call's counts on the device.
struct AnalysisChunk {
    uint32_t grid, block, lds, n_batches;
    uint64_t m, first_sim, stride;
    uint32_t seed_lo, seed_hi;
    uint64_t grid_cap;                      // blocks of a counting kernel the device holds at once (count_grid_x)
    const mcgp::KParams *kp;
    const mcgp::ResumeState *st;            // zero from the grid
    const Layout *ws;
    const std::vector<CountSeg> *segs;
    unsigned long long *count(size_t i) const { return ws->count(i); }
    // ... NULL for a segment that is not wanted
    unsigned long long *wanted(size_t i) const { return (*segs)[i].dst ? ws->count(i) : nullptr; }
};

// What the checked arguments give: known once the parameter block and the state have been accepted.
struct AnalysisPlan {
    std::vector<CountSeg> segs;             // the call's counts, hist [n][n] first
    uint64_t sim_bytes;                     // staged per simulation, out of the kind's budget
    size_t count_lds = 0;                   // dynamic LDS of its counting kernel's block (0: none to check)
    const void *count_fn = nullptr;         // that kernel, where it may need more than the default limit
};

// What mcgp_run_trace, mcgp_run_gaps, mcgp_run_conditions, mcgp_run_stints, mcgp_run_moves and mcgp_run_pit_windows each
// have of their own;
// run_analysis has the rest.
struct AnalysisKind {
    const char *what;                       // the call in check_deviates_32's message
    // generic_geometry's name of the race kernel (and the counting kernel's in the LDS message), note_launch's name
    const char *geo_name, *kernel_name;
    // the instantiation that runs, chosen where its type is known; its register count shapes the launch
    KernelFn kernel;
    uint64_t budget;                        // bytes of staging (kTraceStageBytes ...)
    // the output beside hist_out that must be given, and its name; NULL name: a call from the grid only (mcgp_run_trace),
    // which has checked its pointers with its own message
    const char *required_name;
    const uint64_t *required_out;
    // the call's own checks: behind the source, before the parameter block / behind it (n is checked), before the state
    std::function<int()> check_args, check_fields;
    std::function<AnalysisPlan(uint32_t L, uint32_t lap)> plan;          // lap: the state's, 0 from the grid
    std::function<void(Layout &, uint64_t stride)> regions;              // its staging and its tables
    std::function<int(const AnalysisChunk &)> launch;                    // the race kernel and its counting kernels
};

int32_t run_analysis(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                     uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                     const AnalysisKind &k)
{
    // ---- every argument is checked before any device is looked up
    int rc = MCGP_OK;
    if (k.required_name) {
        if (!hist_out) return fail(MCGP_E_BAD_ARG, "hist_out is NULL");
        if (!k.required_out) return fail(MCGP_E_BAD_ARG, std::string(k.required_name) + " is NULL");
        rc = check_source(grid_probs, state);
        if (rc != MCGP_OK) return rc;
    }
    if (k.check_args && (rc = k.check_args()) != MCGP_OK) return rc;
    std::vector<mcgp::KParams> kps(1);
    mcgp::KParams &kp = kps[0];
    rc = build_params_32(cfg, drv, grid_probs, n, k.what, &kp);
    if (rc != MCGP_OK) return rc;
    if (k.check_fields && (rc = k.check_fields()) != MCGP_OK) return rc;
    const uint32_t L = (uint32_t)cfg->total_laps;
    mcgp::ResumeState st;
    rc = pack_state(state, n, (int)L, 0, &st);
    if (rc != MCGP_OK) return rc;
    if (n_sims == 0) return MCGP_OK;
    const AnalysisPlan p = k.plan(L, state ? (uint32_t)st.lap : 0u);
    Counts counts;
    rc = on_device(device, true, [&](DeviceCtx &c) -> int {
        const uint64_t chunk = stage_chunk_rounds(c, n, k.kernel, k.budget, p.sim_bytes, n_sims);
        // workspace: the kind's staging of one chunk, in rows of `stride` items (a multiple of 256: whole, aligned words
        // for the counting kernels), and its tables | parameter block | state | the counts
        AnalysisChunk a = {};
        a.stride = (chunk + 255) / 256 * 256;
        Layout ws;
        k.regions(ws, a.stride);
        ws.add(&a.kp, 1, &kp);
        if (k.required_name) ws.add(&a.st, 1, &st);
        ws.counts(p.segs);
        const int r = ws.commit(c.work);
        if (r != MCGP_OK) return r;
        if (p.count_lds > c.lds_per_block)
            return fail(MCGP_E_HIP, std::string("the ") + k.geo_name + " counting kernel's block needs " +
                                        std::to_string(p.count_lds) + " bytes of LDS, the device offers " +
                                        std::to_string(c.lds_per_block) + " per block");
        if (p.count_fn)
            HIP_TRY(hipFuncSetAttribute(p.count_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_per_block));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k.kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)c.lds_per_block));
        a.ws = &ws, a.segs = &p.segs;
        a.seed_lo = (uint32_t)seed, a.seed_hi = (uint32_t)(seed >> 32);
        a.grid_cap = (uint64_t)c.cu_count * 8;
        return staged_run(c, k.kernel, k.geo_name, k.kernel_name, n, 1, n_sims, chunk, ws, counts,
                          [&](uint64_t done, uint64_t m, uint32_t grid, uint32_t block, uint32_t lds, uint32_t n_batches) -> int {
            a.grid = grid, a.block = block, a.lds = lds, a.n_batches = n_batches, a.m = m, a.first_sim = sim_offset + done;
            return k.launch(a);
        });
    });
    if (rc != MCGP_OK) return rc;
    counts.add_to(p.segs);
    return MCGP_OK;
}

// The bin edges of mcgp_run_gaps and mcgp_run_pit_windows: 1 to 63, finite, the first above 0, strictly increasing ...
int check_gap_edges(uint32_t n_edges, const double *edges)
{
    if (n_edges < 1 || n_edges > mcgp::kMaxGapEdges) return fail(MCGP_E_BAD_ARG, "n_edges must be in [1, 63]");
    if (!edges) return fail(MCGP_E_BAD_ARG, "edges is NULL");
    for (uint32_t i = 0; i < n_edges; ++i) {
        if (!std::isfinite(edges[i])) return fail(MCGP_E_BAD_ARG, "edges[" + std::to_string(i) + "] is not finite");
        if (i == 0 && !(edges[0] > 0.0)) return fail(MCGP_E_BAD_ARG, "edges[0] must be > 0");
        if (i > 0 && !(edges[i] > edges[i - 1]))
            return fail(MCGP_E_BAD_ARG, "edges[" + std::to_string(i) + "] must be above edges[" + std::to_string(i - 1) + "]");
    }
    return MCGP_OK;
}

// ... and the device's table of them: the call's edges, then +inf to kGapEdgeSlots (gaps.hip.h: gap_bin).
void fill_edge_table(double *table, uint32_t n_edges, const double *edges)
{
    for (uint32_t i = 0; i < mcgp::kGapEdgeSlots; ++i) table[i] = i < n_edges ? edges[i] : HUGE_VAL;
}

}  // namespace

extern "C" {

int32_t mcgp_abi_version(void) { return MCGP_ABI_VERSION; }

// Identity of the sources this binary was compiled from (csrc/source_hash.py, passed in by the Makefile).  The same
// value sits in the file as the text after "MCGP_BUILD_HASH=", so that a loader can read it without mapping the library.
#ifndef MCGP_SOURCE_HASH
#define MCGP_SOURCE_HASH "unknown"
#endif
extern const char mcgp_build_hash_marker[];
__attribute__((used)) const char mcgp_build_hash_marker[] = "MCGP_BUILD_HASH=" MCGP_SOURCE_HASH;
const char *mcgp_build_hash(void) { return mcgp_build_hash_marker + sizeof("MCGP_BUILD_HASH=") - 1; }

int32_t mcgp_device_count(void) { return device_count_nothrow(); }

const char *mcgp_last_error(void) { return g_err.c_str(); }

int32_t mcgp_run_device(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device,
                        void *stream, uint64_t *d_hist, uint8_t *d_orders)
{
    if (!grid_probs || !d_hist) return fail(MCGP_E_BAD_ARG, "grid_probs / d_hist is NULL");
    mcgp::KParams *kp = new (std::nothrow) mcgp::KParams;
    if (!kp) return fail(MCGP_E_NOMEM, "host allocation failed");
    int rc = build_params(cfg, drv, grid_probs, n, kp);
    if (rc == MCGP_OK)
        rc = on_device(device, false, [&](DeviceCtx &c) {
            return launch(c, *kp, n_sims, sim_offset, seed, (hipStream_t)stream,
                          reinterpret_cast<unsigned long long *>(d_hist), d_orders, nullptr);
        });
    delete kp;
    return rc;
}

int32_t mcgp_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                 uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                 uint8_t *orders_out)
{
    if (!grid_probs || !hist_out) return fail(MCGP_E_BAD_ARG, "grid_probs / hist_out is NULL");
    mcgp::KParams *kp = new (std::nothrow) mcgp::KParams;
    if (!kp) return fail(MCGP_E_NOMEM, "host allocation failed");
    int rc = build_params(cfg, drv, grid_probs, n, kp);
    Counts counts;
    if (rc == MCGP_OK)
        rc = on_device(device, false, [&](DeviceCtx &c) -> int {
            HIP_TRY(hipMemsetAsync(c.d_hist, 0, sizeof(unsigned long long) * n * n, nullptr));
            // per-simulation orders are staged in chunks so the device buffer stays bounded
            const uint64_t chunk = orders_out ? kOrdersChunk : n_sims;
            if (orders_out) {
                const int r = c.work.reserve((size_t)std::min(chunk, n_sims) * n);
                if (r != MCGP_OK) return r;
            }
            uint8_t *d_orders = orders_out ? c.work.at<uint8_t>() : nullptr;
            for (uint64_t done = 0; done < n_sims; done += chunk) {
                const uint64_t m = (n_sims - done) < chunk ? (n_sims - done) : chunk;
                const int r = launch(c, *kp, m, sim_offset + done, seed, nullptr, c.d_hist, d_orders, nullptr);
                if (r != MCGP_OK) return r;
                if (d_orders) {
                    const hipError_t e = hipMemcpy(orders_out + (size_t)done * n, d_orders, (size_t)m * n, hipMemcpyDeviceToHost);
                    if (e != hipSuccess) return fail(MCGP_E_HIP, std::string("hipMemcpy(orders): ") + hipGetErrorString(e));
                }
            }
            return counts.download(c.d_hist, (size_t)n * n);
        });
    delete kp;
    if (rc == MCGP_OK) counts.add_to({{hist_out, (size_t)n * n}});
    return rc;
}

int32_t mcgp_simulate_race(const mcgp_config *cfg, const mcgp_drivers *drv, const uint8_t *grid, uint32_t n,
                           uint64_t sim_id, uint64_t seed, int32_t device, uint8_t *order_out)
{
    if (!grid || !order_out) return fail(MCGP_E_BAD_ARG, "grid / order_out is NULL");
    if (n >= 1 && n <= MCGP_MAX_CARS) {
        uint32_t seen = 0;
        for (uint32_t p = 0; p < n; ++p) {
            if (grid[p] >= n || (seen >> grid[p] & 1u)) return fail(MCGP_E_BAD_ARG, "grid is not a permutation of 0..n-1");
            seen |= 1u << grid[p];
        }
    }
    mcgp::KParams *kp = new (std::nothrow) mcgp::KParams;
    if (!kp) return fail(MCGP_E_NOMEM, "host allocation failed");
    int rc = build_params(cfg, drv, nullptr, n, kp);
    if (rc == MCGP_OK)
        rc = on_device(device, false, [&](DeviceCtx &c) -> int {
            HIP_TRY(hipMemcpy(c.d_grid, grid, n, hipMemcpyHostToDevice));
            HIP_TRY(hipMemsetAsync(c.d_hist, 0, sizeof(unsigned long long) * n * n, nullptr));
            const int r = launch(c, *kp, 1, sim_id, seed, nullptr, c.d_hist, c.d_order1, c.d_grid);
            if (r != MCGP_OK) return r;
            const hipError_t e = hipMemcpy(order_out, c.d_order1, n, hipMemcpyDeviceToHost);
            return e == hipSuccess ? MCGP_OK : fail(MCGP_E_HIP, std::string("hipMemcpy(order): ") + hipGetErrorString(e));
        });
    delete kp;
    return rc;
}

// Uploads the front-end inputs of one call into the context's buffers (NULL stream: ordered before what follows).
static int upload_front_end(DeviceCtx &c, const double *rating, const double *teammate_delta, const double *form_score,
                            const double *circuit_affinity, const int32_t *penalty, uint32_t n)
{
    if (!rating || !teammate_delta || !form_score || !circuit_affinity || !penalty)
        return fail(MCGP_E_BAD_ARG, "a front-end input array is NULL");
    if (n < 1 || n > MCGP_MAX_CARS) return fail(MCGP_E_BAD_ARG, "n must be in [1, 32]");
    double in[4 * MCGP_MAX_CARS];
    for (uint32_t d = 0; d < n; ++d) {
        // a non-finite input makes the softmax (inf - inf) or the row adjustments NaN: the race kernel would then
        // sample uniform grids silently, where mcgp_run rejects such a matrix
        if (!std::isfinite(rating[d]) || !std::isfinite(teammate_delta[d]) || !std::isfinite(form_score[d]) ||
            !std::isfinite(circuit_affinity[d]))
            return fail(MCGP_E_BAD_ARG, "a front-end input (rating / teammate_delta / form_score / circuit_affinity) "
                                        "is not finite");
        in[d] = rating[d];
        in[n + d] = teammate_delta[d];
        in[2 * n + d] = form_score[d];
        in[3 * n + d] = circuit_affinity[d];
    }
    HIP_TRY(hipMemcpy(c.d_fe_in, in, sizeof(double) * 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c.d_fe_pen, penalty, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    return MCGP_OK;
}

int32_t mcgp_grid_probs(const double *quali_rating, const double *teammate_delta, const double *form_score,
                        const double *circuit_affinity, const int32_t *penalty, uint32_t n, int32_t device,
                        double *grid_probs_out)
{
    if (!grid_probs_out) return fail(MCGP_E_BAD_ARG, "grid_probs_out is NULL");
    return on_device(device, false, [&](DeviceCtx &c) -> int {
        const int r = upload_front_end(c, quali_rating, teammate_delta, form_score, circuit_affinity, penalty, n);
        if (r != MCGP_OK) return r;
        hipLaunchKernelGGL(grid_probs_kernel, dim3(1), dim3(mcgp::kMaxCars), 0, nullptr, c.d_fe_in, c.d_fe_pen, (int)n,
                           c.d_fe_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(grid_probs_out, c.d_fe_out, sizeof(double) * n * n, hipMemcpyDeviceToHost));
        return MCGP_OK;
    });
}

int32_t mcgp_elo_season(uint32_t n_drivers, uint32_t n_events, const int32_t *kind, const double *k,
                        const uint32_t *count, const uint8_t *who, const double *value, double *ratings,
                        double *after_out, int32_t device)
{
    const uint32_t n = n_drivers;
    if (n < 1 || n > MCGP_MAX_CARS) return fail(MCGP_E_BAD_ARG, "n_drivers must be in [1, 32]");
    if (!ratings) return fail(MCGP_E_BAD_ARG, "ratings is NULL");
    if (n_events > 0 && (!kind || !k || !count || !who || !value)) return fail(MCGP_E_BAD_ARG, "an event array is NULL");
    for (uint32_t i = 0; i < 2 * n; ++i)
        if (!std::isfinite(ratings[i])) return fail(MCGP_E_BAD_ARG, "non-finite rating");
    for (uint32_t e = 0; e < n_events; ++e) {
        if (kind[e] != 0 && kind[e] != 1) return fail(MCGP_E_BAD_ARG, "event kind must be 0 (qualifying) or 1 (race)");
        if (!std::isfinite(k[e])) return fail(MCGP_E_BAD_ARG, "non-finite K factor");
        if (count[e] > n) return fail(MCGP_E_BAD_ARG, "more entries than drivers in an event");
        uint32_t seen = 0;
        for (uint32_t j = 0; j < count[e]; ++j) {
            const uint32_t d = who[(size_t)e * n + j];
            if (d >= n) return fail(MCGP_E_BAD_ARG, "driver index out of range in an event");
            if (seen & (1u << d)) return fail(MCGP_E_BAD_ARG, "a driver is listed twice in one event");
            seen |= 1u << d;
            if (!std::isfinite(value[(size_t)e * n + j])) return fail(MCGP_E_BAD_ARG, "non-finite lap time / position");
        }
    }
    // one buffer for everything the kernel reads and writes, packed on the host: one upload, one launch, one
    // download (the call is latency-bound: a season is a few hundred events for one wavefront)
    const size_t ne = n_events, row = n;
    const size_t o_rat = 0, o_after = o_rat + 2 * row * 8, o_k = o_after + (after_out ? ne * 2 * row * 8 : 0);
    const size_t o_val = o_k + ne * 8, o_kind = o_val + ne * row * 8, o_cnt = o_kind + ne * 4, o_who = o_cnt + ne * 4;
    const size_t bytes = o_who + ne * row;
    std::vector<unsigned char> host(bytes - o_k + 2 * row * 8);        // [ratings | inputs]: the after block is output only
    const size_t in0 = 2 * row * 8;                                    // inputs start here in `host`, at o_k on the device
    std::memcpy(host.data(), ratings, 2 * row * 8);
    if (ne) {
        std::memcpy(host.data() + in0 + (o_k - o_k), k, ne * 8);
        std::memcpy(host.data() + in0 + (o_val - o_k), value, ne * row * 8);
        std::memcpy(host.data() + in0 + (o_kind - o_k), kind, ne * 4);
        std::memcpy(host.data() + in0 + (o_cnt - o_k), count, ne * 4);
        std::memcpy(host.data() + in0 + (o_who - o_k), who, ne * row);
    }
    return on_device(device, false, [&](DeviceCtx &c) -> int {
        const int r = c.work.reserve(bytes);
        if (r != MCGP_OK) return r;
        unsigned char *d = c.work.at();
        HIP_TRY(hipMemcpy(d + o_rat, host.data(), 2 * row * 8, hipMemcpyHostToDevice));
        if (ne) HIP_TRY(hipMemcpy(d + o_k, host.data() + in0, bytes - o_k, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(elo_season_kernel, dim3(1), dim3(mcgp::kMaxCars * mcgp::kMaxCars), 0, nullptr, (int)n, (int)n_events,
                           reinterpret_cast<const int32_t *>(d + o_kind), reinterpret_cast<const double *>(d + o_k),
                           reinterpret_cast<const uint32_t *>(d + o_cnt), d + o_who,
                           reinterpret_cast<const double *>(d + o_val), reinterpret_cast<double *>(d + o_rat),
                           after_out ? reinterpret_cast<double *>(d + o_after) : nullptr);
        HIP_TRY(hipGetLastError());
        if (after_out && ne) {
            // ratings and the snapshots are adjacent: one download
            std::vector<double> back(2 * row + ne * 2 * row);
            HIP_TRY(hipMemcpy(back.data(), d + o_rat, back.size() * 8, hipMemcpyDeviceToHost));
            std::memcpy(ratings, back.data(), 2 * row * 8);
            std::memcpy(after_out, back.data() + 2 * row, ne * 2 * row * 8);
        } else {
            HIP_TRY(hipMemcpy(ratings, d + o_rat, 2 * row * 8, hipMemcpyDeviceToHost));
        }
        return MCGP_OK;
    });
}

int32_t mcgp_run_from_ratings(const mcgp_config *cfg, const mcgp_drivers *drv, const double *quali_rating,
                              const double *teammate_delta, const double *form_score,
                              const double *circuit_affinity, const int32_t *penalty, uint32_t n, uint64_t n_sims,
                              uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                              double *grid_probs_out)
{
    if (!hist_out) return fail(MCGP_E_BAD_ARG, "hist_out is NULL");
    mcgp::KParams *kp = new (std::nothrow) mcgp::KParams;
    if (!kp) return fail(MCGP_E_NOMEM, "host allocation failed");
    int rc = build_params(cfg, drv, nullptr, n, kp);               // grid_probs slot left zero: the device fills it
    Counts counts;
    if (rc == MCGP_OK)
        rc = on_device(device, false, [&](DeviceCtx &c) -> int {
            int r = upload_front_end(c, quali_rating, teammate_delta, form_score, circuit_affinity, penalty, n);
            if (r != MCGP_OK) return r;
            HIP_TRY(hipMemsetAsync(c.d_hist, 0, sizeof(unsigned long long) * n * n, nullptr));
            FrontEnd fe;
            fe.on = true;
            r = launch(c, *kp, n_sims, sim_offset, seed, nullptr, c.d_hist, nullptr, nullptr, fe);
            if (r == MCGP_OK) r = counts.download(c.d_hist, (size_t)n * n);
            if (r != MCGP_OK || !grid_probs_out) return r;
            // the matrix the race kernel sampled from, recomputed by the same kernel from the same inputs into the
            // context's scratch matrix (the parameter block itself is not read back)
            hipLaunchKernelGGL(grid_probs_kernel, dim3(1), dim3(mcgp::kMaxCars), 0, nullptr, c.d_fe_in, c.d_fe_pen, (int)n,
                               c.d_fe_out);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(grid_probs_out, c.d_fe_out, sizeof(double) * n * n, hipMemcpyDeviceToHost));
            return MCGP_OK;
        });
    delete kp;
    if (rc == MCGP_OK) counts.add_to({{hist_out, (size_t)n * n}});
    return rc;
}

int32_t mcgp_run_batch(uint32_t n_problems, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                       const double *const *grid_probs, uint32_t n, uint64_t n_sims, const uint64_t *sim_offsets,
                       const uint64_t *seeds, int32_t device, uint64_t *hist_out)
{
    if (!cfgs || !drvs || !grid_probs || !seeds || !hist_out) return fail(MCGP_E_BAD_ARG, "a batch array is NULL");
    if (n_problems < 1 || n_problems > 4096) return fail(MCGP_E_BAD_ARG, "n_problems must be in [1, 4096]");
    if (n_sims >= 0xFFFFFE00ull) return fail(MCGP_E_BAD_ARG, "n_sims per problem must be below 2^32 - 512 in a batch");
    if (n_sims == 0) return MCGP_OK;
    // Every problem gets what mcgp_run would give it (reference src/validation.py:179-185: a sweep is a loop over
    // independent predictions, none of which can make another one fail).  The problems the batch kernel takes -- the
    // register kernel's domain at the default deviate width -- share ONE launch; the others (deviates = 53, a problem only
    // the generic kernel serves, everything under MCGP_FORCE_GENERIC=1) run one after the other through the single-problem
    // path, inside this call, into the same output.
    std::vector<mcgp::KParams> kps;                  // the problems of the shared launch, compacted
    std::vector<mcgp::BatchItem> items;
    std::vector<uint32_t> shared_index, solo_index;  // original indices
    std::vector<mcgp::KParams> solo_kps;
    const bool generic = force_generic();
    const RegKernels *rk = reg_kernels(n);
    {
        mcgp::KParams kp;
        for (uint32_t p = 0; p < n_problems; ++p) {
            if (!grid_probs[p]) return fail(MCGP_E_BAD_ARG, "a grid_probs pointer of the batch is NULL");
            int rc = build_params(&cfgs[p], &drvs[p], grid_probs[p], n, &kp);
            if (rc == MCGP_OK) rc = check_wide(kp);
            if (rc != MCGP_OK) return rc;
            if (!rk || generic || kp.wide || !mcgp::reg_kernel_serves(kp)) {
                solo_index.push_back(p);
                solo_kps.push_back(kp);
            } else {
                shared_index.push_back(p);
                kps.push_back(kp);
                items.push_back(mcgp::BatchItem{sim_offsets ? sim_offsets[p] : 0ull, seeds[p]});
            }
        }
    }
    const uint32_t n_shared = (uint32_t)kps.size();
    const size_t cells = (size_t)n * n;
    // the parameter blocks of the shared launch as the kernel reads them: `param_stride` bytes apart, each with its
    // problem's retirement table behind it (build_retire_table; room for the largest: the problems may differ in laps)
    size_t param_stride = 0;
    for (const mcgp::KParams &k : kps) param_stride = std::max(param_stride, mcgp::retire_table_bytes(k.n, k.total_laps, false));
    param_stride = mcgp::kRetireTabOffset + (param_stride + 255) / 256 * 256;
    std::vector<unsigned char> blocks(param_stride * n_shared);
    for (uint32_t j = 0; j < n_shared; ++j) {
        std::memcpy(blocks.data() + param_stride * j, &kps[j], sizeof(mcgp::KParams));
        mcgp::build_retire_table(kps[j], false, blocks.data() + param_stride * j + mcgp::kRetireTabOffset);
    }
    Counts counts;
    const int rc = on_device(device, true, [&](DeviceCtx &c) -> int {
        // geometry of the shared launch: the register kernel's block, one more LDS word that names the block's next problem
        const int waves = mcgp::reg_block_waves((int)n);
        const uint32_t block = (uint32_t)waves * 64u;
        const size_t lds = mcgp::shared_lds_bytes_reg((int)n) + (size_t)block * mcgp::per_thread_lds_bytes_reg((int)n) +
                           mcgp::kBatchLdsExtra;
        // The batch kernel is built in the default block shape only.  On a device that offers less LDS per block than that
        // block needs there is no shared launch: its problems run one after the other through launch(), like the solo ones
        // and into the same histograms, in blocks of kSmallBlockWaves waves -- or fail with launch()'s error when not even
        // those fit (mcgp_last_kernel_name / mcgp_last_launch_info then describe the last of these launches).
        const bool shared_launch = n_shared != 0 && lds <= c.lds_per_block;
        int reg_cap = 4 * mcgp::reg_min_waves((int)n);
        int blocks_per_cu = (int)(c.lds_per_block / lds);
        if (blocks_per_cu * waves > reg_cap) blocks_per_cu = reg_cap / waves;
        if (blocks_per_cu < 1) blocks_per_cu = 1;
        const uint32_t n_chunks = (uint32_t)((n_sims + 63) / 64);
        // no more blocks than the batch has wave-chunks to fill them with
        const uint64_t n_tasks = ((uint64_t)n_shared * n_chunks + (uint64_t)waves - 1) / (uint64_t)waves;
        uint64_t grid = (uint64_t)c.cu_count * (uint64_t)blocks_per_cu;
        if (grid > n_tasks) grid = n_tasks;
        if (!shared_launch) grid = 0;                                           // (no lanes, no retirement lists)
        // workspace: parameter blocks with their retirement tables | items | histograms (the shared launch's problems, then
        // the solo ones) | one ticket counter per problem of the shared launch | its lanes' retirement lists
        Layout ws;
        const size_t o_kps = ws.add(blocks.size()), o_items = ws.add(sizeof(mcgp::BatchItem) * n_shared);
        const size_t o_hist = ws.add(sizeof(unsigned long long) * cells * n_problems);
        const size_t o_ticket = ws.add(sizeof(uint32_t) * n_shared);
        const size_t o_retire = ws.add(mcgp::reg_retire_ws_bytes((int)n, (size_t)grid * block));
        int r = c.work.reserve(ws.bytes);
        if (r != MCGP_OK) return r;
        unsigned long long *d_hist = c.work.at<unsigned long long>(o_hist);
        HIP_TRY(hipMemsetAsync(d_hist, 0, o_retire - o_hist, nullptr));         // the histograms and ticket counters
        if (shared_launch) {
            const BatchKernelFn kernel = rk->batch;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)c.lds_per_block));
            HIP_TRY(hipMemcpyAsync(c.work.at(o_kps), blocks.data(), blocks.size(), hipMemcpyHostToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(c.work.at(o_items), items.data(), sizeof(mcgp::BatchItem) * n_shared, hipMemcpyHostToDevice,
                                   nullptr));
            hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(block), lds, nullptr, c.work.at<const mcgp::KParams>(o_kps),
                               c.work.at<const mcgp::BatchItem>(o_items), n_shared, n_sims, d_hist, n_chunks,
                               c.work.at<uint32_t>(o_ticket), c.work.at<uint32_t>(o_retire), (uint32_t)param_stride);
            HIP_TRY(hipGetLastError());
            note_launch(c, (uint32_t)grid, block, (uint32_t)lds, "mcgp::race_kernel_reg_batch<%u>", n);
        } else {
            for (uint32_t j = 0; j < n_shared; ++j) {
                r = launch(c, kps[j], n_sims, items[j].sim_offset, items[j].seed, nullptr, d_hist + (size_t)j * cells, nullptr,
                           nullptr);
                if (r != MCGP_OK) return r;
            }
        }
        // the problems that run by themselves: exactly mcgp_run's path, one after the other (null stream)
        for (size_t j = 0; j < solo_index.size(); ++j) {
            const uint32_t p = solo_index[j];
            r = launch(c, solo_kps[j], n_sims, sim_offsets ? sim_offsets[p] : 0ull, seeds[p], nullptr,
                       d_hist + (n_shared + j) * cells, nullptr, nullptr);
            if (r != MCGP_OK) return r;
        }
        return counts.download(d_hist, cells * n_problems);
    });
    if (rc != MCGP_OK) return rc;
    std::vector<Counts::Seg> segs;                  // in the order of the histograms on the device
    for (uint32_t p : shared_index) segs.push_back({hist_out + (size_t)p * cells, cells});
    for (uint32_t p : solo_index) segs.push_back({hist_out + (size_t)p * cells, cells});
    counts.add_to(segs);
    return MCGP_OK;
}

// The per-round outputs of mcgp_run_championship_rounds (NULL for mcgp_run_championship: no per-round kernel runs).
struct ChampRoundsOut {
    uint64_t *round_hist, *contend, *secure, *team_round_hist, *team_contend, *team_secure;
};

// The fastest-lap bonuses of mcgp_run_championship_bonus (NULL for the other two calls: no race has one).
struct ChampBonus {
    const int32_t *points, *within;         // [R] each
    uint64_t *bonus_hist, *fastest_hist;    // [R][n] each, or NULL
};

// What mcgp_run_championship_live adds (NULL for the other three calls: race 0 from the grid, no conditional table).
struct ChampLive {
    const mcgp_race_state *state0;      // NULL: race 0 from the grid
    int32_t given_race;                 // -1: no conditional table
    uint64_t *title_given;              // [n][n][n], NULL exactly when given_race == -1
};

// mcgp_run_championship (rounds == NULL), mcgp_run_championship_rounds, mcgp_run_championship_bonus and
// mcgp_run_championship_live: one body, so that the four season outputs of the calls come from the same launches.  A race
// without a bonus goes through launch(); a race with one runs race_fastest_kernel (fastest.hip.h) on the same chunk, and
// champ_bonus behind its champ_accumulate.  With live->state0, race 0 is race_resume_kernel's of that one state
// (resume.hip.h); with live->given_race >= 0 that race's orders go to a staging buffer of their own, which champ_given
// (champ_given.hip.h) reads behind the chunk's champ_rank.  Without `live` the launches are what they always were.
static int32_t run_championship(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                uint64_t *gain_hist, uint64_t *race_hist, const ChampRoundsOut *rounds,
                                const ChampBonus *bonus = nullptr, const ChampLive *live = nullptr)
{
    const mcgp_race_state *state0 = live ? live->state0 : nullptr;
    const int32_t given_race = live ? live->given_race : -1;
    // ---- every argument is checked before any device is looked up
    if (rounds) {
        if (!rounds->round_hist) return fail(MCGP_E_BAD_ARG, "round_hist is NULL");
        if (!rounds->contend) return fail(MCGP_E_BAD_ARG, "contend_out is NULL");
        if (!rounds->secure) return fail(MCGP_E_BAD_ARG, "secure_out is NULL");
        const int given = (rounds->team_round_hist != nullptr) + (rounds->team_contend != nullptr) + (rounds->team_secure != nullptr);
        if (given != 0 && given != 3)
            return fail(MCGP_E_BAD_ARG, "team_round_hist, team_contend_out and team_secure_out must be all given or all NULL");
    }
    if (!cfgs || !drvs || !grid_probs || !seeds || !points || !countback || !team || !champ_hist || !team_hist ||
        !gain_hist)
        return fail(MCGP_E_BAD_ARG, "a championship array is NULL");
    if (n_races < 1 || n_races > (uint32_t)mcgp::kChampMaxRaces) return fail(MCGP_E_BAD_ARG, "n_races must be in [1, 64]");
    if (n < 1 || n > MCGP_MAX_CARS) return fail(MCGP_E_BAD_ARG, "n must be in [1, 32]");
    if (n_teams < 1 || n_teams > n) return fail(MCGP_E_BAD_ARG, "n_teams must be in [1, n]");
    for (uint32_t d = 0; d < n; ++d)
        if (team[d] < 0 || (uint32_t)team[d] >= n_teams) return fail(MCGP_E_BAD_ARG, "a team index is outside [0, n_teams)");
    if (given_race < -1 || given_race >= (int32_t)n_races)
        return fail(MCGP_E_BAD_ARG, "given_race = " + std::to_string(given_race) + " is outside [-1, n_races - 1]");
    if (live && given_race == -1 && live->title_given)
        return fail(MCGP_E_BAD_ARG, "title_given_out must be NULL when given_race is -1");
    if (live && given_race >= 0 && !live->title_given)
        return fail(MCGP_E_BAD_ARG, "title_given_out is NULL (given_race names a race)");
    constexpr uint64_t kMaxPoints = (1u << mcgp::kChampPointsBits) - 1, kMaxCount = (1u << mcgp::kChampCountBits) - 1;
    uint64_t G = 0, awarded = 0;         // most points one driver can gain in these races; points the races award in all
    uint32_t n_cb = 0;                   // countback races
    for (uint32_t r = 0; r < n_races; ++r) {
        if (countback[r] > 1) return fail(MCGP_E_BAD_ARG, "countback[r] must be 0 or 1");
        n_cb += countback[r];
        int64_t best = 0;
        for (uint32_t p = 0; p < n; ++p) {
            const int32_t v = points[(size_t)r * n + p];
            if (v < 0) return fail(MCGP_E_BAD_ARG, "a points-table entry is negative");
            if ((uint64_t)v > kMaxPoints) return fail(MCGP_E_BAD_ARG, "a points-table entry is above 65535, the limit of a driver's total points");
            if (v > best) best = v;
            awarded += (uint64_t)v;
        }
        G += (uint64_t)best;
    }
    if (bonus && (!bonus->points || !bonus->within)) return fail(MCGP_E_BAD_ARG, "bonus_points / bonus_within is NULL");
    bool any_bonus = false;
    for (uint32_t r = 0; r < n_races && bonus; ++r) {
        const int32_t b = bonus->points[r], w = bonus->within[r];
        if (b < 0 || (uint64_t)b > kMaxPoints)
            return fail(MCGP_E_BAD_ARG, "bonus_points[" + std::to_string(r) + "] = " + std::to_string(b) + " is outside [0, 65535]");
        if (b == 0) continue;                               // (bonus_within is ignored where there is no bonus)
        if (w < 1 || (uint32_t)w > n)
            return fail(MCGP_E_BAD_ARG, "bonus_within[" + std::to_string(r) + "] = " + std::to_string(w) + " is outside [1, n]");
        any_bonus = true;
        G += (uint64_t)b;
        awarded += (uint64_t)b;
    }
    for (uint32_t d = 0; d < n; ++d) {
        const int64_t ip = init_points ? init_points[d] : 0;
        if (ip < 0) return fail(MCGP_E_BAD_ARG, "an initial points total is negative");
        if ((uint64_t)ip + G > kMaxPoints)
            return fail(MCGP_E_BAD_ARG, "a driver's total points (initial points plus the most these races award, " +
                                            std::to_string((uint64_t)ip + G) + ") may exceed the limit of 65535");
        for (uint32_t p = 0; p < n; ++p) {
            const int64_t ic = init_counts ? init_counts[(size_t)d * n + p] : 0;
            if (ic < 0) return fail(MCGP_E_BAD_ARG, "an initial countback count is negative");
            if ((uint64_t)ic + n_cb > kMaxCount)
                return fail(MCGP_E_BAD_ARG, "a driver's count of finishes in one position (initial count plus countback "
                                            "races, " + std::to_string((uint64_t)ic + n_cb) + ") may exceed the limit of 31");
        }
    }
    std::vector<mcgp::KParams> kps(n_races);
    mcgp::ResumeState st0;
    std::memset(&st0, 0, sizeof(st0));
    for (uint32_t r = 0; r < n_races; ++r) {
        if (r == 0 && state0) {
            // race 0 from a state: mcgp_run_from_state's checks of one state, with its messages
            if (grid_probs[0]) return fail(MCGP_E_BAD_ARG, "grid_probs[0] must be NULL when state0 is given");
            int rc = build_params_32(&cfgs[0], &drvs[0], nullptr, n, "a resumed race runs", &kps[0]);
            if (rc != MCGP_OK) return rc;
            if (any_bonus && bonus->points[0] > 0)
                return fail(MCGP_E_BAD_ARG, "bonus_points[0]: a race resumed from a state has no fastest-lap bonus (the laps "
                                            "before the state are unknown)");
            rc = pack_state(state0, n, cfgs[0].total_laps, sim_offset, &st0);
            if (rc != MCGP_OK) return rc;
            continue;
        }
        if (!grid_probs[r]) return fail(MCGP_E_BAD_ARG, "a grid_probs pointer of the championship is NULL");
        int rc = build_params(&cfgs[r], &drvs[r], grid_probs[r], n, &kps[r]);
        if (rc == MCGP_OK) rc = check_wide(kps[r]);
        if (rc != MCGP_OK) return rc;
        if (any_bonus && bonus->points[r] > 0 && kps[r].wide)
            return fail(MCGP_E_BAD_ARG, "bonus_points[" + std::to_string(r) + "]: a race with a bonus runs at MCGP_DEVIATES_32 "
                                        "only (the generic kernel has no 53-bit path)");
    }
    const int32_t *bonus_pts = any_bonus ? bonus->points : nullptr;     // NULL: every race through launch(), as without bonuses
    // ---- key layouts and the kernels' tables (champ_pack.h)
    mcgp::ChampPack pk;
    const std::string pack_err = mcgp::pack_championship(n_races, n, points, countback, init_points, init_counts, team,
                                                         n_teams, G, awarded, n_cb, &pk, bonus_pts);
    if (!pack_err.empty()) return fail(MCGP_E_BAD_ARG, pack_err);
    if (n_sims == 0) return MCGP_OK;
    const uint32_t words = pk.words, team_cbits = pk.team_cbits, team_words = pk.team_words, gain_cols = pk.gain_cols;
    const std::vector<uint8_t> &members = pk.members, &n_members = pk.n_members;
    const std::vector<uint64_t> &init_key = pk.init_key, &add = pk.add;
    const std::vector<int32_t> &init_pts = pk.init_pts;
    const size_t champ_cells = (size_t)n * n, team_cells = (size_t)n_teams * n_teams, gain_cells = (size_t)n * gain_cols;
    const size_t race_cells = race_hist ? (size_t)n_races * n * n : 0;
    // per round: [R][n][n] | [R][n] | [R][n], then the same three for the teams (behind the season's histograms)
    const bool round_teams = rounds && rounds->team_round_hist;
    const uint32_t round_T = round_teams ? n_teams : 0;
    const size_t rh_cells = rounds ? (size_t)n_races * n * n : 0, rc_cells = rounds ? (size_t)n_races * n : 0;
    const size_t trh_cells = (size_t)n_races * round_T * round_T, trc_cells = (size_t)n_races * round_T;
    const size_t round_cells = rh_cells + 2 * rc_cells + trh_cells + 2 * trc_cells;
    // bonus [R][n] | fastest [R][n], behind the per-round counts
    const size_t bonus_cells = bonus_pts ? (size_t)n_races * n : 0;
    // title_given [n][n][n], behind the bonus counts
    const size_t given_cells = given_race >= 0 ? (size_t)n * n * n : 0;
    const size_t hist_cells = champ_cells + team_cells + gain_cells + race_cells + round_cells + 2 * bonus_cells + given_cells;
    std::vector<uint32_t> driver_rem, team_rem;
    if (rounds) mcgp::champ_remaining(n_races, n, points, n_members.data(), n_teams, &driver_rem, &team_rem, bonus_pts);
    // the parameter blocks of the bonus races, in race order (kp_index[r]: the race's block, -1 without a bonus)
    std::vector<mcgp::KParams> bonus_kps;
    std::vector<int> kp_index(n_races, -1);
    for (uint32_t r = 0; r < n_races && bonus_pts; ++r)
        if (bonus_pts[r] > 0) {
            kp_index[r] = (int)bonus_kps.size();
            bonus_kps.push_back(kps[r]);
        }
    Counts counts;
    const int rc = on_device(device, true, [&](DeviceCtx &c) -> int {
        // rank kernel's LDS: the gain histogram joins the block when the block still leaves room for a second one
        const mcgp::ChampRankLds lds_base = mcgp::champ_rank_lds(n, words, n_teams, team_words, gain_cols, false);
        const mcgp::ChampRankLds lds_gain = mcgp::champ_rank_lds(n, words, n_teams, team_words, gain_cols, true);
        const bool gain_in_lds = lds_gain.bytes <= c.lds_per_block / 2;
        const uint32_t rank_lds = gain_in_lds ? lds_gain.bytes : lds_base.bytes;
        if (rank_lds > c.lds_per_block)
            return fail(MCGP_E_HIP, "the standings kernel needs " + std::to_string(rank_lds) + " bytes of LDS, the device offers " +
                                        std::to_string(c.lds_per_block) + " per block");
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::champ_rank),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)rank_lds));
        const uint32_t round_lds = rounds ? mcgp::champ_round_lds(n, words, round_T, team_words).bytes : 0;
        if (round_lds > c.lds_per_block)
            return fail(MCGP_E_HIP, "the per-round standings kernel needs " + std::to_string(round_lds) +
                                        " bytes of LDS, the device offers " + std::to_string(c.lds_per_block) + " per block");
        if (rounds)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::champ_round),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)round_lds));
        const KernelFn fast_fn = reinterpret_cast<KernelFn>(&mcgp::race_fastest_kernel);   // (for its register count)
        if (bonus_pts)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::race_fastest_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_per_block));
        // champ_given's table: in the block's LDS when it fits the budget next to the tile, else by global atomics.
        // MCGP_LDS_PER_BLOCK is read per call here, as mcgp_run_matchups reads it.
        const size_t given_budget = lds_limit(c.lds_per_block);
        const bool given_in_lds = mcgp::champ_given_lds(n, true).bytes <= given_budget;
        const uint32_t given_lds = mcgp::champ_given_lds(n, given_in_lds).bytes;
        if (given_cells) {
            if (given_lds > given_budget)
                return fail(MCGP_E_HIP, "the title-by-finish kernel needs " + std::to_string(given_lds) +
                                            " bytes of LDS, the device offers " + std::to_string(given_budget) + " per block");
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::champ_given),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)given_lds));
        }
        const KernelFn resume_fn = reinterpret_cast<KernelFn>(&mcgp::race_resume_kernel);   // (for its register count)
        // workspace: orders staging of one chunk | the chunk's standing keys | tables | histograms | the bonus races'
        // parameter blocks | the chunk's fastest-lap bytes (two rows of the chunk's capacity) | the given race's orders
        // of the chunk | the resumed race's parameter block and state
        const uint64_t cap = std::min(n_sims, kOrdersChunk);
        Layout ws;
        const size_t o_orders = ws.add(cap * n), o_keys = ws.add((size_t)words * n * cap * 8), o_add = ws.add(add.size() * 8);
        const size_t o_init = ws.add(init_key.size() * 8), o_mem = ws.add(members.size()), o_nmem = ws.add(n_teams);
        const size_t o_ipts = ws.add(4 * n), o_trem = ws.add(4 * team_rem.size()), o_hist = ws.add(hist_cells * 8);
        const size_t o_bkp = ws.add(sizeof(mcgp::KParams) * bonus_kps.size()), o_fl = ws.add(bonus_pts ? 2 * cap : 0);
        const size_t o_keep = ws.add(given_cells ? cap * n : 0), o_lkp = ws.add(state0 ? sizeof(mcgp::KParams) : 0);
        const size_t o_lst = ws.add(state0 ? sizeof(mcgp::ResumeState) : 0);
        int r = c.work.reserve(ws.bytes);
        if (r != MCGP_OK) return r;
        uint8_t *d_orders = c.work.at<uint8_t>(o_orders);
        uint64_t *d_keys = c.work.at<uint64_t>(o_keys);
        uint8_t *d_fl = c.work.at<uint8_t>(o_fl);
        unsigned long long *h_champ = c.work.at<unsigned long long>(o_hist), *h_team = h_champ + champ_cells;
        unsigned long long *h_gain = h_team + team_cells, *h_race = h_gain + gain_cells;
        unsigned long long *h_round = h_race + race_cells, *h_contend = h_round + rh_cells, *h_secure = h_contend + rc_cells;
        unsigned long long *h_tround = h_secure + rc_cells, *h_tcontend = h_tround + trh_cells, *h_tsecure = h_tcontend + trc_cells;
        unsigned long long *h_bonus = h_tsecure + trc_cells, *h_fastest = h_bonus + bonus_cells;
        unsigned long long *h_given = h_fastest + bonus_cells;
        uint8_t *d_keep = c.work.at<uint8_t>(o_keep);
        if (state0) {
            HIP_TRY(hipMemcpyAsync(c.work.at(o_lkp), &kps[0], sizeof(mcgp::KParams), hipMemcpyHostToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(c.work.at(o_lst), &st0, sizeof(mcgp::ResumeState), hipMemcpyHostToDevice, nullptr));
        }
        if (!bonus_kps.empty())
            HIP_TRY(hipMemcpyAsync(c.work.at(o_bkp), bonus_kps.data(), sizeof(mcgp::KParams) * bonus_kps.size(),
                                   hipMemcpyHostToDevice, nullptr));
        if (!team_rem.empty())
            HIP_TRY(hipMemcpyAsync(c.work.at(o_trem), team_rem.data(), 4 * team_rem.size(), hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(c.work.at(o_add), add.data(), add.size() * 8, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(c.work.at(o_init), init_key.data(), init_key.size() * 8, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(c.work.at(o_mem), members.data(), members.size(), hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(c.work.at(o_nmem), n_members.data(), n_teams, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(c.work.at(o_ipts), init_pts.data(), 4 * n, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(h_champ, 0, hist_cells * 8, nullptr));
        // without race_hist the race kernels count into the context's scratch histogram (not read back)
        HIP_TRY(hipMemsetAsync(c.d_hist, 0, sizeof(unsigned long long) * n * n, nullptr));
        const uint64_t acc_cap = (uint64_t)c.cu_count * 8;
        uint64_t rank_per_cu = c.lds_per_block / rank_lds;
        if (rank_per_cu > 8) rank_per_cu = 8;
        if (rank_per_cu < 1) rank_per_cu = 1;
        const uint64_t rank_cap = (uint64_t)c.cu_count * rank_per_cu;
        uint64_t round_per_cu = rounds ? c.lds_per_block / round_lds : 1;
        if (round_per_cu > 8) round_per_cu = 8;
        const uint64_t round_cap = (uint64_t)c.cu_count * round_per_cu;
        uint64_t given_per_cu = given_budget / given_lds;
        if (given_per_cu > 8) given_per_cu = 8;
        const uint64_t given_cap = (uint64_t)c.cu_count * given_per_cu;
        for (uint64_t done = 0; done < n_sims; done += cap) {
            const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
            // chunk-outer, race-inner: every race of the chunk through mcgp_run's own launch path, its orders into the
            // staging buffer, then folded into the keys before the next race overwrites them
            for (uint32_t rr = 0; rr < n_races; ++rr) {
                unsigned long long *h_this = race_hist ? h_race + (size_t)rr * n * n : c.d_hist;
                // the given race's orders outlive the race loop: they go to a buffer no other race writes
                uint8_t *d_ord = (int32_t)rr == given_race ? d_keep : d_orders;
                if (rr == 0 && state0) {
                    // mcgp_run_from_state's launch of one state (m <= 2^22: one launch); ids st0.sim_offset + done + i
                    uint32_t grid = 0, block = 0, lds = 0;
                    r = generic_geometry(c, resume_fn, "resume", n, m, &grid, &block, &lds);
                    if (r != MCGP_OK) return r;
                    const uint64_t n_batches = (m + block - 1) / block;
                    hipLaunchKernelGGL(mcgp::race_resume_kernel, dim3(grid, 1), dim3(block), lds, nullptr,
                                       c.work.at<const mcgp::KParams>(o_lkp), c.work.at<const mcgp::ResumeState>(o_lst), m, done,
                                       (uint32_t)seeds[0], (uint32_t)(seeds[0] >> 32), h_this, d_ord, (uint32_t)n_batches);
                    HIP_TRY(hipGetLastError());
                    note_launch(c, grid, block, lds, "mcgp::race_resume_kernel");
                } else if (kp_index[rr] < 0) {
                    r = launch(c, kps[rr], m, sim_offset + done, seeds[rr], nullptr, h_this, d_ord, nullptr);
                    if (r != MCGP_OK) return r;
                } else {
                    // the generic kernel's block shape and LDS (m <= 2^22: one launch)
                    uint32_t grid = 0, block = 0, lds = 0;
                    r = generic_geometry(c, fast_fn, "fastest-lap", n, m, &grid, &block, &lds);
                    if (r != MCGP_OK) return r;
                    const uint64_t n_batches = (m + block - 1) / block;
                    hipLaunchKernelGGL(mcgp::race_fastest_kernel, dim3(grid), dim3(block), lds, nullptr,
                                       c.work.at<const mcgp::KParams>(o_bkp) + kp_index[rr], m, sim_offset + done,
                                       (uint32_t)seeds[rr], (uint32_t)(seeds[rr] >> 32), h_this, d_ord, d_fl, d_fl + cap,
                                       (uint32_t)n_batches);
                    HIP_TRY(hipGetLastError());
                    note_launch(c, grid, block, lds, "mcgp::race_fastest_kernel");
                }
                const uint64_t tiles = (m + mcgp::kChampAccBlock - 1) / mcgp::kChampAccBlock;
                hipLaunchKernelGGL(mcgp::champ_accumulate, dim3((uint32_t)std::min(tiles, acc_cap)), dim3(mcgp::kChampAccBlock), 0,
                                   nullptr, d_ord, m, n, words, cap, d_keys,
                                   c.work.at<const uint64_t>(o_add) + (size_t)rr * n * words, c.work.at<const uint64_t>(o_init),
                                   rr == 0 ? 1u : 0u);
                HIP_TRY(hipGetLastError());
                if (kp_index[rr] >= 0) {
                    hipLaunchKernelGGL(mcgp::champ_bonus, dim3((uint32_t)std::min(tiles, acc_cap)), dim3(mcgp::kChampAccBlock), 0,
                                       nullptr, d_fl, d_fl + cap, m, n, words, cap, d_keys, pk.bonus_add[rr],
                                       (uint32_t)bonus->within[rr], h_fastest + (size_t)rr * n, h_bonus + (size_t)rr * n);
                    HIP_TRY(hipGetLastError());
                }
                if (rounds) {
                    // the standings as they now are, before the next race adds to them
                    const uint64_t rtiles = (m + mcgp::kChampTile - 1) / mcgp::kChampTile;
                    hipLaunchKernelGGL(mcgp::champ_round, dim3((uint32_t)std::min(rtiles, round_cap)),
                                       dim3(mcgp::kChampRoundBlock), round_lds, nullptr, d_keys, m, cap, n, words, round_T,
                                       team_words, team_cbits, c.work.at<const uint8_t>(o_mem), c.work.at<const uint8_t>(o_nmem),
                                       driver_rem[rr], c.work.at<const uint32_t>(o_trem) + (size_t)rr * n_teams,
                                       rr + 1 == n_races ? 1u : 0u, h_round + (size_t)rr * n * n, h_contend + (size_t)rr * n,
                                       h_secure + (size_t)rr * n, h_tround + (size_t)rr * round_T * round_T,
                                       h_tcontend + (size_t)rr * round_T, h_tsecure + (size_t)rr * round_T);
                    HIP_TRY(hipGetLastError());
                }
            }
            const uint64_t tiles = (m + mcgp::kChampTile - 1) / mcgp::kChampTile;
            hipLaunchKernelGGL(mcgp::champ_rank, dim3((uint32_t)std::min(tiles, rank_cap)), dim3(mcgp::kChampRankBlock), rank_lds,
                               nullptr, d_keys, m, cap, n, words, n_teams, team_words, team_cbits, c.work.at<const uint8_t>(o_mem),
                               c.work.at<const uint8_t>(o_nmem), c.work.at<const int32_t>(o_ipts), gain_cols, gain_in_lds ? 1u : 0u,
                               h_champ, h_team, h_gain);
            HIP_TRY(hipGetLastError());
            if (given_cells) {
                // the chunk's final keys and the kept orders, before the next chunk starts both afresh
                const uint64_t gtiles = (m + mcgp::kChampGivenBlock - 1) / mcgp::kChampGivenBlock;
                hipLaunchKernelGGL(mcgp::champ_given, dim3((uint32_t)std::min(gtiles, given_cap)), dim3(mcgp::kChampGivenBlock),
                                   given_lds, nullptr, d_keys, d_keep, m, cap, n, words, given_in_lds ? 1u : 0u, h_given);
                HIP_TRY(hipGetLastError());
                // (its dynamic LDS tells the two modes apart: the tile alone, or the tile and the table)
                note_launch(c, (uint32_t)std::min(gtiles, given_cap), mcgp::kChampGivenBlock, given_lds, "mcgp::champ_given");
            }
        }
        return counts.download(h_champ, hist_cells);
    });
    if (rc != MCGP_OK) return rc;
    std::vector<Counts::Seg> segs = {{champ_hist, champ_cells}, {team_hist, team_cells}, {gain_hist, gain_cells},
                                     {race_hist, race_cells}};
    if (rounds) {
        segs.push_back({rounds->round_hist, rh_cells});
        segs.push_back({rounds->contend, rc_cells});
        segs.push_back({rounds->secure, rc_cells});
        segs.push_back({rounds->team_round_hist, trh_cells});
        segs.push_back({rounds->team_contend, trc_cells});
        segs.push_back({rounds->team_secure, trc_cells});
    }
    if (bonus) {
        segs.push_back({bonus->bonus_hist, bonus_cells});
        segs.push_back({bonus->fastest_hist, bonus_cells});
    }
    if (given_cells) segs.push_back({live->title_given, given_cells});      // (without `bonus` there are no bonus cells)
    counts.add_to(segs);
    return MCGP_OK;
}

int32_t mcgp_run_championship(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                              const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                              const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                              const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                              uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                              uint64_t *gain_hist, uint64_t *race_hist)
{
    return run_championship(n_races, cfgs, drvs, grid_probs, n, n_sims, sim_offset, seeds, points, countback, init_points,
                            init_counts, team, n_teams, device, champ_hist, team_hist, gain_hist, race_hist, nullptr);
}

int32_t mcgp_run_championship_rounds(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                     const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                     const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                     const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                     uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                     uint64_t *gain_hist, uint64_t *race_hist, uint64_t *round_hist, uint64_t *contend_out,
                                     uint64_t *secure_out, uint64_t *team_round_hist, uint64_t *team_contend_out,
                                     uint64_t *team_secure_out)
{
    const ChampRoundsOut rounds = {round_hist, contend_out, secure_out, team_round_hist, team_contend_out, team_secure_out};
    return run_championship(n_races, cfgs, drvs, grid_probs, n, n_sims, sim_offset, seeds, points, countback, init_points,
                            init_counts, team, n_teams, device, champ_hist, team_hist, gain_hist, race_hist, &rounds);
}

int32_t mcgp_run_championship_bonus(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                    const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                    const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                    const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                    uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                    uint64_t *gain_hist, uint64_t *race_hist, uint64_t *round_hist, uint64_t *contend_out,
                                    uint64_t *secure_out, uint64_t *team_round_hist, uint64_t *team_contend_out,
                                    uint64_t *team_secure_out, const int32_t *bonus_points, const int32_t *bonus_within,
                                    uint64_t *bonus_hist, uint64_t *fastest_hist)
{
    const ChampRoundsOut rounds = {round_hist, contend_out, secure_out, team_round_hist, team_contend_out, team_secure_out};
    const ChampBonus bonus = {bonus_points, bonus_within, bonus_hist, fastest_hist};
    const bool by_round = round_hist || contend_out || secure_out;      // all three NULL: no per-round work
    if (!by_round && (team_round_hist || team_contend_out || team_secure_out))
        return fail(MCGP_E_BAD_ARG, "team_round_hist, team_contend_out and team_secure_out need round_hist, contend_out and "
                                    "secure_out");
    return run_championship(n_races, cfgs, drvs, grid_probs, n, n_sims, sim_offset, seeds, points, countback, init_points,
                            init_counts, team, n_teams, device, champ_hist, team_hist, gain_hist, race_hist,
                            by_round ? &rounds : nullptr, &bonus);
}

int32_t mcgp_run_championship_live(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                   const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                   const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                   const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                   uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                   uint64_t *gain_hist, uint64_t *race_hist, uint64_t *round_hist, uint64_t *contend_out,
                                   uint64_t *secure_out, uint64_t *team_round_hist, uint64_t *team_contend_out,
                                   uint64_t *team_secure_out, const int32_t *bonus_points, const int32_t *bonus_within,
                                   uint64_t *bonus_hist, uint64_t *fastest_hist, const mcgp_race_state *state0,
                                   int32_t given_race, uint64_t *title_given_out)
{
    const ChampRoundsOut rounds = {round_hist, contend_out, secure_out, team_round_hist, team_contend_out, team_secure_out};
    const ChampBonus bonus = {bonus_points, bonus_within, bonus_hist, fastest_hist};
    const ChampLive live = {state0, given_race, title_given_out};
    const bool by_round = round_hist || contend_out || secure_out;      // all three NULL: no per-round work
    if (!by_round && (team_round_hist || team_contend_out || team_secure_out))
        return fail(MCGP_E_BAD_ARG, "team_round_hist, team_contend_out and team_secure_out need round_hist, contend_out and "
                                    "secure_out");
    const bool with_bonus = bonus_points || bonus_within;               // both NULL: no bonus anywhere
    return run_championship(n_races, cfgs, drvs, grid_probs, n, n_sims, sim_offset, seeds, points, countback, init_points,
                            init_counts, team, n_teams, device, champ_hist, team_hist, gain_hist, race_hist,
                            by_round ? &rounds : nullptr, with_bonus ? &bonus : nullptr, &live);
}

int32_t mcgp_run_matchups(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                          uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                          uint64_t *ahead_out, uint64_t *podium_out)
{
    // ---- every argument is checked before any device is looked up
    if (!grid_probs || !hist_out || !ahead_out) return fail(MCGP_E_BAD_ARG, "grid_probs / hist_out / ahead_out is NULL");
    std::vector<mcgp::KParams> kps(1);
    mcgp::KParams &kp = kps[0];
    int rc = build_params(cfg, drv, grid_probs, n, &kp);
    if (rc != MCGP_OK) return rc;
    if (podium_out && n < 3) return fail(MCGP_E_BAD_ARG, "podium_out needs n >= 3 (pass NULL to skip the podium counts)");
    rc = check_wide(kp);
    if (rc != MCGP_OK) return rc;
    if (n_sims == 0) return MCGP_OK;
    // hist [n][n] | ahead [n][n] | podium [n][n][n]
    const std::vector<Counts::Seg> segs = {{hist_out, (size_t)n * n}, {ahead_out, (size_t)n * n},
                                           {podium_out, podium_out ? (size_t)n * n * n : 0}};
    Counts counts;
    rc = on_device(device, true, [&](DeviceCtx &c) -> int {
        // block shape: the widest block whose LDS fits the device's budget, with the podium table in LDS if any block
        // can hold it, else with the podium counted by global atomics.  MCGP_LDS_PER_BLOCK (a device that offers less)
        // is read per call here, so that a test reaches the global-atomic path in a process whose context exists.
        const size_t budget = lds_limit(c.lds_per_block);
        uint32_t mode = podium_out ? mcgp::kPodiumLds : mcgp::kPodiumNone, block = 0;
        auto widest = [&](bool podium_in_lds) -> uint32_t {
            for (uint32_t b = mcgp::kMatchMaxBlock; b >= 64; b /= 2)
                if (mcgp::match_lds(n, b, podium_in_lds).bytes <= budget) return b;
            return 0;
        };
        block = widest(mode == mcgp::kPodiumLds);
        if (!block && mode == mcgp::kPodiumLds) {
            mode = mcgp::kPodiumGlobal;
            block = widest(false);
        }
        if (!block)
            return fail(MCGP_E_HIP, "the matchups kernel needs " + std::to_string(mcgp::match_lds(n, 64, false).bytes) +
                                        " bytes of LDS, the device offers " + std::to_string(budget) + " per block");
        const uint32_t lds = mcgp::match_lds(n, block, mode == mcgp::kPodiumLds).bytes;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcgp::race_matchups),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        // workspace: orders staging of one chunk | the counts
        const uint64_t cap = std::min<uint64_t>(n_sims, mcgp::kMatchMaxSims);
        uint8_t *d_orders;
        Layout ws;
        ws.add(&d_orders, cap * n);
        ws.counts(segs);
        int r = ws.commit(c.work);
        if (r != MCGP_OK) return r;
        uint64_t per_cu = budget / lds;
        if (per_cu > 8) per_cu = 8;
        if (per_cu < 1) per_cu = 1;
        const uint64_t grid_cap = (uint64_t)c.cu_count * per_cu;
        for (uint64_t done = 0; done < n_sims; done += cap) {
            const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
            // the chunk's race through mcgp_run's own launch path (the position histogram is counted there), its
            // orders into the staging buffer, then counted before the next chunk overwrites them
            r = launch(c, kp, m, sim_offset + done, seed, nullptr, ws.count(0), d_orders, nullptr);
            if (r != MCGP_OK) return r;
            const uint64_t tiles = (m + block - 1) / block;
            hipLaunchKernelGGL(mcgp::race_matchups, dim3((uint32_t)std::min(tiles, grid_cap)), dim3(block), lds, nullptr,
                               d_orders, m, n, mode, ws.count(1), podium_out ? ws.count(2) : nullptr);
            HIP_TRY(hipGetLastError());
        }
        return counts.download(ws);
    });
    if (rc != MCGP_OK) return rc;
    counts.add_to(segs);
    return MCGP_OK;
}

int32_t mcgp_run_from_state(const mcgp_config *cfg, const mcgp_drivers *drv, uint32_t n, uint32_t n_states,
                            const mcgp_race_state *states, uint64_t n_sims, const uint64_t *sim_offsets, uint64_t seed,
                            int32_t device, uint64_t *hist_out, uint8_t *orders_out)
{
    // ---- every argument is checked before any device is looked up
    if (!hist_out) return fail(MCGP_E_BAD_ARG, "hist_out is NULL");
    if (!states) return fail(MCGP_E_BAD_ARG, "states is NULL");
    if (n_states < 1 || n_states > mcgp::kMaxResumeStates) return fail(MCGP_E_BAD_ARG, "n_states must be in [1, 4096]");
    std::vector<mcgp::KParams> kps(1);
    mcgp::KParams &kp = kps[0];
    int rc = build_params_32(cfg, drv, nullptr, n, "a resumed race runs", &kp);
    if (rc != MCGP_OK) return rc;
    std::vector<mcgp::ResumeState> st(n_states);
    for (uint32_t si = 0; si < n_states; ++si) {
        const std::string err = mcgp::pack_race_state(states[si], si, n, cfg->total_laps, &st[si]);
        if (!err.empty()) return fail(MCGP_E_BAD_ARG, err);
        st[si].sim_offset = sim_offsets ? sim_offsets[si] : 0;
    }
    if (n_sims == 0) return MCGP_OK;
    const size_t cells = (size_t)n_states * n * n;
    Counts counts;
    rc = on_device(device, true, [&](DeviceCtx &c) -> int {
        // simulations per launch: at most max_sims_per_launch() per state (u32 block counts), and with orders at most
        // kOrdersChunk over all states
        uint64_t chunk = max_sims_per_launch();
        if (orders_out) chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(1, kOrdersChunk / n_states));
        const uint64_t cap = n_sims < chunk ? n_sims : chunk;
        // workspace: orders staging | parameter block | states | histograms
        uint8_t *d_orders;
        const mcgp::KParams *d_kp;
        const mcgp::ResumeState *d_st;
        Layout ws;
        ws.add(&d_orders, orders_out ? (size_t)n_states * cap * n : 0);
        ws.add(&d_kp, 1, &kp);
        ws.add(&d_st, n_states, st.data());
        ws.counts({{hist_out, cells}});
        int r = ws.commit(c.work);
        if (r != MCGP_OK) return r;
        if (!orders_out) d_orders = nullptr;
        unsigned long long *d_h = ws.count(0);
        const KernelFn geo_fn = reinterpret_cast<KernelFn>(&mcgp::race_resume_kernel);   // (for its register count)
        uint32_t grid = 0, block = 0, lds = 0;
        for (uint64_t done = 0; done < n_sims; done += cap) {
            const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
            // the generic kernel's block shape; the blocks the device holds at once are shared out over the states
            r = generic_geometry(c, geo_fn, "resume", n, m, &grid, &block, &lds);
            if (r != MCGP_OK) return r;
            const uint64_t n_batches = (m + block - 1) / block;
            const uint32_t gx = (grid + n_states - 1) / n_states;
            hipLaunchKernelGGL(mcgp::race_resume_kernel, dim3(gx, n_states), dim3(block), lds, nullptr, d_kp, d_st, m, done,
                               (uint32_t)seed, (uint32_t)(seed >> 32), d_h, d_orders, (uint32_t)n_batches);
            HIP_TRY(hipGetLastError());
            if (orders_out)
                HIP_TRY(hipMemcpy2D(orders_out + (size_t)done * n, (size_t)n_sims * n, d_orders, (size_t)m * n,
                                    (size_t)m * n, n_states, hipMemcpyDeviceToHost));
            grid = gx * n_states;
        }
        note_launch(c, grid, block, lds, "mcgp::race_resume_kernel");
        return counts.download(d_h, cells);
    });
    if (rc != MCGP_OK) return rc;
    counts.add_to({{hist_out, cells}});
    return MCGP_OK;
}

int32_t mcgp_run_trace(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                       uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                       uint64_t *lap_pos_out, uint64_t *laps_led_out, uint64_t *stops_out, uint64_t *fastest_out,
                       uint64_t *events_out)
{
    if (!grid_probs || !hist_out || !lap_pos_out) return fail(MCGP_E_BAD_ARG, "grid_probs / hist_out / lap_pos_out is NULL");
    uint32_t L = 0, rows = 0;
    uint8_t *d_stage;
    uint64_t *d_rec;
    AnalysisKind k = {"a trace runs", "trace", "mcgp::race_trace_kernel", reinterpret_cast<KernelFn>(&mcgp::race_trace_kernel),
                      kTraceStageBytes};
    k.plan = [&](uint32_t laps, uint32_t) {
        L = laps, rows = L * n;
        const size_t c_laps = (size_t)n * (L + 1);
        // hist [n][n] | lap_pos [L][n][n + 1] | laps_led [n][L + 1] | stops [n][L + 1] | fastest [n] | events [3][L + 1]
        return AnalysisPlan{{{hist_out, (size_t)n * n}, {lap_pos_out, (size_t)rows * (n + 1)}, {laps_led_out, c_laps},
                             {stops_out, c_laps}, {fastest_out, n}, {events_out, 3 * (size_t)(L + 1)}},
                            rows};
    };
    // staging of one chunk, L n rows of `stride` bytes | the chunk's records
    k.regions = [&](Layout &ws, uint64_t stride) {
        ws.add(&d_stage, (size_t)rows * stride);
        ws.add(&d_rec, (size_t)stride);
    };
    k.launch = [&](const AnalysisChunk &a) -> int {
        hipLaunchKernelGGL(mcgp::race_trace_kernel, dim3(a.grid), dim3(a.block), a.lds, nullptr, a.kp, a.m, a.first_sim, a.seed_lo,
                           a.seed_hi, a.count(0), d_stage, a.stride, d_rec, a.n_batches);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(mcgp::trace_count_positions, dim3((uint32_t)std::min<uint64_t>(rows, a.grid_cap)),
                           dim3(mcgp::kTraceCountBlock), 0, nullptr, d_stage, a.stride, a.m, rows, n, a.count(1));
        HIP_TRY(hipGetLastError());
        if (laps_led_out || stops_out) {
            hipLaunchKernelGGL(mcgp::trace_count_laps, dim3(count_grid_x((a.m + 3) / 4, mcgp::kTraceCountBlock, a.grid_cap, n), n),
                               dim3(mcgp::kTraceCountBlock), 2 * (size_t)(L + 1) * 4, nullptr, d_stage, a.stride, a.m, n, L,
                               a.count(2), a.count(3));
            HIP_TRY(hipGetLastError());
        }
        if (fastest_out || events_out) {
            hipLaunchKernelGGL(mcgp::trace_count_records, dim3(count_grid_x(a.m, mcgp::kTraceCountBlock, a.grid_cap, 1)),
                               dim3(mcgp::kTraceCountBlock), ((size_t)mcgp::kMaxCars + 3 * (size_t)(L + 1)) * 4, nullptr, d_rec,
                               a.m, n, L, a.count(4), a.count(5));
            HIP_TRY(hipGetLastError());
        }
        return MCGP_OK;
    };
    return run_analysis(cfg, drv, grid_probs, nullptr, n, n_sims, sim_offset, seed, device, hist_out, k);
}

int32_t mcgp_run_strategies(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                            const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                            const mcgp_pit_plan *plans, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                            int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint8_t *orders_out)
{
    ScenarioKind k = {"strategies run", "strategy", "mcgp::race_strategy_kernel", 0u};
    k.sim_bytes = n;                        // a position byte per driver
    // every scenario but the first against the first: S - 1 grid rows (never run for one scenario)
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *) {
        hipLaunchKernelGGL(mcgp::strategy_count_deltas,
                           dim3(count_grid_x(l.m, mcgp::kStrategyCountBlock, grid_cap, l.S - 1), l.S - 1),
                           dim3(mcgp::kStrategyCountBlock), 0, nullptr, l.stage, l.m, n, d_delta);
    };
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_penalties(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                           const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                           const mcgp_pit_plan *plans, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                           uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                           uint64_t *delta_out, uint64_t *fate_out, uint8_t *orders_out)
{
    std::vector<mcgp::PenaltyScenario> pens;
    std::vector<mcgp::PenaltyLap> pen_laps;
    ScenarioKind k = {"penalties run", "penalties", "mcgp::race_penalties_kernel", mcgp::kRulePenalties};
    k.tables = {{"penalty_count", "penalties", penalty_count, penalties, [&](uint64_t *n_pens) {
        return mcgp::check_penalty_counts(n_scenarios, penalty_count, n_pens);
    }}};
    k.pack = [&](int first_lap, bool resumed) {
        return mcgp::pack_penalties(n_scenarios, penalty_count, penalties, n, cfg->total_laps, first_lap, resumed, &pens,
                                    &pen_laps);
    };
    k.sim_bytes = n;                        // a byte per driver: its position, and the fate of its penalty above it
    k.pos_mask = mcgp::kStagePosMask;
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t) {
        ws.add(&l.pn, n_scenarios, pens.data());
        ws.add(&l.nl, pen_laps.size(), pen_laps.data());
    };
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        count_penalties(l, n, grid_cap, d_delta, extra[0]);
    };
    // fate [S][n][4]; column 0 (no SERVE_AT_STOP penalty) is, like delta's centre bin, what the others leave of n_sims
    k.outputs = {fate_output(fate_out)};
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_events(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                        const mcgp_pit_plan *plans, const uint32_t *event_count, const mcgp_lap_event *events,
                        uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                        uint64_t *delta_out, uint64_t *events_out, uint8_t *orders_out)
{
    std::vector<uint8_t> event_laps;
    ScenarioKind k = {"events run", "events", "mcgp::race_events_kernel", mcgp::kRuleEvents};
    k.tables = {{"event_count", "events", event_count, events, [&](uint64_t *n_events) {
        return mcgp::check_event_counts(n_scenarios, event_count, n_events);
    }}};
    k.pack = [&](int first_lap, bool resumed) {
        return mcgp::pack_events(n_scenarios, event_count, events, cfg->total_laps, first_lap, resumed, &event_laps);
    };
    // positions and event counts of a chunk share the strategy call's budget: n + 4 bytes per scenario and simulation
    k.sim_bytes = (size_t)n + 4;
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t chunk) {
        ws.add(&l.evs, (size_t)n_scenarios * chunk);
        ws.add(&l.el, event_laps.size(), event_laps.data());
    };
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        count_events(l, n, (uint32_t)cfg->total_laps, grid_cap, d_delta, extra[0]);
    };
    k.outputs = {events_output(events_out)};
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_paces(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                       const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                       const mcgp_pit_plan *plans, const uint32_t *pace_count, const mcgp_pace_offset *paces,
                       uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                       uint64_t *delta_out, uint64_t *carried_out, uint8_t *orders_out)
{
    std::vector<mcgp::PaceScenario> pscen;
    std::vector<mcgp::PaceLap> pace_laps;
    std::vector<double> lap_sec;
    ScenarioKind k = {"paces run", "paces", "mcgp::race_paces_kernel", mcgp::kRulePaces};
    k.tables = {{"pace_count", "paces", pace_count, paces, [&](uint64_t *n_paces) {
        return mcgp::check_pace_counts(n_scenarios, pace_count, n_paces);
    }}};
    // lap 1 reads the base pace too: from the grid an offset may name it
    k.pack = [&](int first_lap, bool resumed) {
        return mcgp::pack_paces(n_scenarios, pace_count, paces, n, cfg->total_laps, resumed ? first_lap : 1, resumed, &pscen,
                                &pace_laps, &lap_sec);
    };
    // a position byte per driver, and its u16 of laps carried when they are counted
    k.sim_bytes = carried_out ? (size_t)n * 3 : (size_t)n;
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t chunk) {
        if (carried_out) ws.add(&l.car, (size_t)n_scenarios * chunk * n);
        ws.add(&l.ps, n_scenarios, pscen.data());
        ws.add(&l.pl, pace_laps.size(), pace_laps.data());
        ws.add(&l.sec, lap_sec.size(), lap_sec.data());
    };
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        count_paces(l, n, (uint32_t)cfg->total_laps, grid_cap, d_delta, extra[0]);
    };
    k.outputs = {carried_output(carried_out, cfg)};
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_combined(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                          const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                          const mcgp_pit_plan *plans, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                          const uint32_t *event_count, const mcgp_lap_event *events, const uint32_t *pace_count,
                          const mcgp_pace_offset *paces, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                          int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *fate_out, uint64_t *events_out,
                          uint64_t *carried_out, uint8_t *orders_out)
{
    // a NULL count array: none in any scenario (n_scenarios is checked, against the same limit, before a count is read)
    static const uint32_t none[mcgp::kMaxStrategyScenarios] = {};
    if (!penalty_count) penalty_count = none;
    if (!event_count) event_count = none;
    if (!pace_count) pace_count = none;
    std::vector<mcgp::PenaltyScenario> pens;
    std::vector<mcgp::PenaltyLap> pen_laps;
    std::vector<uint8_t> event_laps;
    std::vector<mcgp::PaceScenario> pscen;
    std::vector<mcgp::PaceLap> pace_laps;
    std::vector<double> lap_sec;
    ScenarioKind k = {"combined run", "combined", "mcgp::race_combined_kernel", mcgp::kRuleAll};
    k.tables = {
        {"penalty_count", "penalties", penalty_count, penalties,
         [&](uint64_t *total) { return mcgp::check_penalty_counts(n_scenarios, penalty_count, total); }},
        {"event_count", "events", event_count, events,
         [&](uint64_t *total) { return mcgp::check_event_counts(n_scenarios, event_count, total); }},
        {"pace_count", "paces", pace_count, paces,
         [&](uint64_t *total) { return mcgp::check_pace_counts(n_scenarios, pace_count, total); }},
    };
    // each packer with its own call's first lap: lap 1 reads the base pace, so from the grid an offset may name it
    k.pack = [&](int first_lap, bool resumed) {
        const int L = cfg->total_laps;
        std::string e = mcgp::pack_penalties(n_scenarios, penalty_count, penalties, n, L, first_lap, resumed, &pens, &pen_laps);
        if (e.empty()) e = mcgp::pack_events(n_scenarios, event_count, events, L, first_lap, resumed, &event_laps);
        if (e.empty())
            e = mcgp::pack_paces(n_scenarios, pace_count, paces, n, L, resumed ? first_lap : 1, resumed, &pscen, &pace_laps,
                                 &lap_sec);
        return e;
    };
    // a byte per driver (position | fate << 5), the u32 of event counts and the drivers' u16 of laps carried when wanted
    k.sim_bytes = (size_t)n + (events_out ? 4 : 0) + (carried_out ? (size_t)n * 2 : 0);
    k.pos_mask = mcgp::kStagePosMask;
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t chunk) {
        if (events_out) ws.add(&l.evs, (size_t)n_scenarios * chunk);
        if (carried_out) ws.add(&l.car, (size_t)n_scenarios * chunk * n);
        ws.add(&l.pn, n_scenarios, pens.data());
        ws.add(&l.nl, pen_laps.size(), pen_laps.data());
        ws.add(&l.el, event_laps.size(), event_laps.data());
        ws.add(&l.ps, n_scenarios, pscen.data());
        ws.add(&l.pl, pace_laps.size(), pace_laps.data());
        ws.add(&l.sec, lap_sec.size(), lap_sec.data());
    };
    // the deltas come from penalties_count, the one that masks the fate off the position byte
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        const uint32_t L = (uint32_t)cfg->total_laps;
        if (d_delta || extra[0]) count_penalties(l, n, grid_cap, d_delta, extra[0]);
        if (extra[1]) count_events(l, n, L, grid_cap, nullptr, extra[1]);
        if (extra[2]) count_paces(l, n, L, grid_cap, nullptr, extra[2]);
    };
    k.outputs = {fate_output(fate_out), events_output(events_out), carried_output(carried_out, cfg)};
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_weather(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                         const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                         const mcgp_pit_plan *plans, const uint32_t *change_count, const mcgp_track_change *changes,
                         const mcgp_weather_model *model, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                         int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *wrong_laps_out,
                         uint8_t *orders_out)
{
    std::vector<uint8_t> cond_laps;
    std::vector<double> table;
    ScenarioKind k = {"weather run", "weather", "mcgp::race_weather_kernel", mcgp::kRuleWeather};
    k.tables = {{"change_count", "changes", change_count, changes, [&](uint64_t *n_changes) {
        return mcgp::check_change_counts(n_scenarios, change_count, n_changes);
    }}};
    // the call-wide model is checked with the changes (cfg has been checked by then)
    k.pack = [&](int first_lap, bool resumed) {
        return mcgp::pack_weather(n_scenarios, change_count, changes, model, cfg->track_condition, cfg->total_laps, first_lap,
                                  resumed, &cond_laps, &table);
    };
    // a position byte per driver, and its u16 of laps on the wrong tyres when they are counted
    k.sim_bytes = wrong_laps_out ? (size_t)n * 3 : (size_t)n;
    // the kernel reads the condition bytes and the table through the arguments of the rule sets it never meets
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t chunk) {
        if (wrong_laps_out) ws.add(&l.car, (size_t)n_scenarios * chunk * n);
        ws.add(&l.el, cond_laps.size(), cond_laps.data());
        ws.add(&l.sec, table.size(), table.data());
    };
    // the deltas as mcgp_run_strategies counts them (S - 1 grid rows), the laps on the wrong tyres one layer per driver
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        if (d_delta)
            hipLaunchKernelGGL(mcgp::strategy_count_deltas,
                               dim3(count_grid_x(l.m, mcgp::kStrategyCountBlock, grid_cap, l.S - 1), l.S - 1),
                               dim3(mcgp::kStrategyCountBlock), 0, nullptr, l.stage, l.m, n, d_delta);
        if (extra[0])
            hipLaunchKernelGGL(mcgp::weather_count,
                               dim3(count_grid_x(l.m, mcgp::kWeatherCountBlock, grid_cap, (uint64_t)l.S * n), l.S, n),
                               dim3(mcgp::kWeatherCountBlock), 0, nullptr, l.car, l.m, n, (uint32_t)cfg->total_laps, extra[0]);
    };
    // wrong_laps [S][n][L + 1]; column 0 is, like carried's, what the others leave of n_sims
    k.outputs = {carried_output(wrong_laps_out, cfg)};
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_grids(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                       uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                       const uint32_t *edit_count, const mcgp_grid_edit *edits, uint64_t n_sims, uint64_t sim_offset,
                       uint64_t seed, int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *start_out,
                       uint64_t *gain_out, uint8_t *orders_out)
{
    std::vector<mcgp::GridScenario> grids;
    ScenarioKind k = {"grids run", "grids", "mcgp::race_grids_kernel", mcgp::kRuleGrid};
    k.tables = {{"edit_count", "edits", edit_count, edits, [&](uint64_t *n_edits) {
        return mcgp::check_edit_counts(n_scenarios, edit_count, n, n_edits);
    }}};
    k.pack = [&](int, bool) { return mcgp::pack_grids(n_scenarios, edit_count, edits, n, &grids); };
    // a position byte per driver, and its u16 start slot when the start slots or the gains are counted
    const bool want_start = start_out || gain_out;
    k.sim_bytes = want_start ? (size_t)n * 3 : (size_t)n;
    // the kernel reads the edit table through the argument of a rule set it never meets
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t chunk) {
        if (want_start) ws.add(&l.car, (size_t)n_scenarios * chunk * n);
        ws.add(&l.gr, grids.size(), grids.data());
    };
    // the deltas as mcgp_run_strategies counts them (S - 1 grid rows), the start slots and gains one layer per driver
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        if (d_delta)
            hipLaunchKernelGGL(mcgp::strategy_count_deltas,
                               dim3(count_grid_x(l.m, mcgp::kStrategyCountBlock, grid_cap, l.S - 1), l.S - 1),
                               dim3(mcgp::kStrategyCountBlock), 0, nullptr, l.stage, l.m, n, d_delta);
        if (extra[0] || extra[1])
            hipLaunchKernelGGL(mcgp::grid_count,
                               dim3(count_grid_x(l.m, mcgp::kGridCountBlock, grid_cap, (uint64_t)l.S * n), l.S, n),
                               dim3(mcgp::kGridCountBlock), 0, nullptr, l.stage, l.car, l.m, n, extra[0], extra[1]);
    };
    // start [S][n][n] and gain [S][n][2n - 1]: every cell is counted, neither needs a fix-up
    k.outputs = {{start_out, [](size_t S, size_t n, size_t) { return S * n * n; }, nullptr},
                 {gain_out, [](size_t S, size_t n, size_t) { return S * n * (2 * n - 1); }, nullptr}};
    return run_scenarios(cfg, drv, grid_probs, nullptr, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_priors(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                        const mcgp_pit_plan *plans, const uint32_t *prior_count, const mcgp_pace_prior *priors,
                        uint32_t n_edges, const double *edges, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                        int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *draws_out, float *offsets_out,
                        uint8_t *orders_out)
{
    std::vector<mcgp::PriorScenario> pscen;
    std::vector<float> offsets, back;       // collected on the host, handed over only once everything has run
    ScenarioKind k = {"priors run", "priors", "mcgp::race_priors_kernel", mcgp::kRulePriors};
    // the call-wide edges are checked with the counts, in front of the items
    k.tables = {{"prior_count", "priors", prior_count, priors, [&](uint64_t *n_priors) {
        const std::string e = mcgp::check_prior_counts(n_scenarios, prior_count, n_priors);
        return e.empty() ? mcgp::check_prior_edges(n_edges, edges) : e;
    }}};
    k.pack = [&](int, bool) { return mcgp::pack_priors(n_scenarios, prior_count, priors, n, n_edges, edges, &pscen); };
    // a position byte and a bin byte per driver, and its binary32 offset when the offsets are wanted
    k.sim_bytes = offsets_out ? (size_t)n * 6 : (size_t)n * 2;
    k.lane_lds = mcgp::prior_lane_lds_bytes((int)n);
    // the kernel reads the item table and writes the bins and the offsets through the arguments of rule sets it never meets
    k.regions = [&](Layout &ws, ScenarioChunk &l, uint64_t chunk) {
        if (offsets_out) ws.add(&l.offs, (size_t)n_scenarios * chunk * n);
        ws.add(&l.bins, (size_t)n_scenarios * chunk * n);
        ws.add(&l.pr, pscen.size(), pscen.data());
    };
    // one pass: the deltas' layer (which returns at once when they are not wanted), then (draws wanted) one per driver
    k.count = [&](const ScenarioChunk &l, uint64_t grid_cap, unsigned long long *d_delta, unsigned long long *const *extra) {
        const uint32_t gz = extra[0] ? 1u + n : 1u;
        hipLaunchKernelGGL(mcgp::priors_count,
                           dim3(count_grid_x(l.m, mcgp::kPriorsCountBlock, grid_cap, (uint64_t)l.S * gz), l.S, gz),
                           dim3(mcgp::kPriorsCountBlock), 0, nullptr, l.stage, l.bins, l.m, n, n_edges + 1u, d_delta, extra[0]);
    };
    // draws [S][n][n_edges + 1][n]: every cell is counted, no fix-up
    k.outputs = {{draws_out, [n_edges](size_t S, size_t n, size_t) { return S * n * (n_edges + 1) * n; }, nullptr}};
    if (offsets_out) {
        k.read_back = [&](const ScenarioChunk &l, uint64_t done) -> int {
            if (offsets.empty()) offsets.resize((size_t)n_scenarios * n_sims * n);
            back.resize((size_t)n_scenarios * l.m * n);
            HIP_TRY(hipMemcpy(back.data(), l.offs, back.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (uint32_t si = 0; si < n_scenarios; ++si)
                std::memcpy(offsets.data() + ((size_t)si * n_sims + done) * n, back.data() + (size_t)si * l.m * n,
                            (size_t)l.m * n * sizeof(float));
            return MCGP_OK;
        };
        k.hand_over = [&] { std::memcpy(offsets_out, offsets.data(), offsets.size() * sizeof(float)); };
    }
    return run_scenarios(cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, n_sims, sim_offset, seed, device,
                         hist_out, delta_out, orders_out, k);
}

int32_t mcgp_run_gaps(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                      const mcgp_race_state *state, uint32_t n, uint32_t n_edges, const double *edges, uint32_t n_pairs,
                      const uint8_t *pairs, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device,
                      uint64_t *hist_out, uint64_t *lap_gap_out, uint64_t *lead_out, uint64_t *pair_out)
{
    const auto kernel = state ? &mcgp::race_gaps_kernel<true> : &mcgp::race_gaps_kernel<false>;
    uint32_t L = 0, lap0 = 0, rows = 0;                         // laps lap0 + 1 .. L are recorded
    const uint32_t B = n_edges + 1;
    double edge_table[mcgp::kGapEdgeSlots];                     // the call's edges, then +inf (gaps.hip.h: gap_bin)
    size_t count_lds = 0;
    uint8_t *d_stage;
    const double *d_edges;
    const uint8_t *d_pairs;
    AnalysisKind k = {"gaps run", "gaps", "mcgp::race_gaps_kernel", reinterpret_cast<KernelFn>(kernel), kGapsStageBytes,
                      "lap_gap_out", lap_gap_out};
    k.check_args = [&]() -> int {
        const int rc = check_gap_edges(n_edges, edges);
        if (rc != MCGP_OK) return rc;
        if (n_pairs > mcgp::kMaxGapPairs) return fail(MCGP_E_BAD_ARG, "n_pairs must be in [0, 64]");
        if (n_pairs && !pairs) return fail(MCGP_E_BAD_ARG, "pairs is NULL");
        if (n_pairs && !pair_out) return fail(MCGP_E_BAD_ARG, "pair_out is NULL");
        if (!n_pairs && pair_out) return fail(MCGP_E_BAD_ARG, "pair_out must be NULL when n_pairs is 0");
        return MCGP_OK;
    };
    k.check_fields = [&]() -> int {
        for (uint32_t p = 0; p < n_pairs; ++p) {
            const uint32_t a = pairs[2 * p], b = pairs[2 * p + 1];
            if (a >= n || b >= n)
                return fail(MCGP_E_BAD_ARG, "pairs[" + std::to_string(p) + "]: driver index must be below n");
            if (a == b) return fail(MCGP_E_BAD_ARG, "pairs[" + std::to_string(p) + "]: a pair needs two different drivers");
        }
        return MCGP_OK;
    };
    k.plan = [&](uint32_t laps, uint32_t lap) {
        L = laps, lap0 = lap, rows = (L - lap0) * (n + 1 + n_pairs);
        fill_edge_table(edge_table, n_edges, edges);
        // the counting kernel's columns: 4 x 256 bytes per value, up to 129 values (129 KiB of a CU's 160)
        count_lds = (size_t)(n_pairs ? 2 * B + 1 : B + 1) * mcgp::kGapsCountBlock * 4;
        // hist [n][n] | lap_gap [L][n][B + 1] | lead [L][B + 1] | pair [L][n_pairs][2B + 1].  A race resumed after its
        // last lap records nothing: one row's worth of staging keeps the sizes non-zero
        return AnalysisPlan{{{hist_out, (size_t)n * n}, {lap_gap_out, (size_t)L * n * (B + 1)}, {lead_out, (size_t)L * (B + 1)},
                             {pair_out, (size_t)L * n_pairs * (2 * B + 1)}},
                            std::max<uint64_t>(rows, 1), count_lds, reinterpret_cast<const void *>(&mcgp::gaps_count_rows)};
    };
    // staging of one chunk in rows of `stride` bytes | edges | pairs
    k.regions = [&](Layout &ws, uint64_t stride) {
        ws.add(&d_stage, (size_t)std::max<uint32_t>(rows, 1) * stride);
        ws.add(&d_edges, mcgp::kGapEdgeSlots, edge_table);
        ws.add(&d_pairs, 2 * (size_t)std::max<uint32_t>(n_pairs, 1), n_pairs ? pairs : nullptr);
    };
    k.launch = [&](const AnalysisChunk &a) -> int {
        hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(a.block), a.lds, nullptr, a.kp, a.st, d_edges, n_edges, d_pairs, n_pairs,
                           a.m, a.first_sim, a.seed_lo, a.seed_hi, a.count(0), d_stage, a.stride, a.n_batches);
        HIP_TRY(hipGetLastError());
        if (rows) {
            hipLaunchKernelGGL(mcgp::gaps_count_rows, dim3((uint32_t)std::min<uint64_t>(rows, a.grid_cap)),
                               dim3(mcgp::kGapsCountBlock), count_lds, nullptr, d_stage, a.stride, a.m, rows, n, n_pairs, B,
                               lap0, a.count(1), a.count(2), a.count(3));
            HIP_TRY(hipGetLastError());
        }
        return MCGP_OK;
    };
    return run_analysis(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, k);
}

static_assert(mcgp::kMaxPitWindows == MCGP_MAX_PIT_WINDOWS, "the device's window table holds the C ABI's limit");

int32_t mcgp_run_pit_windows(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                             const mcgp_race_state *state, uint32_t n, uint32_t n_edges, const double *edges,
                             uint32_t n_windows, const uint8_t *window_drivers, const double *window_losses, uint64_t n_sims,
                             uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out, uint64_t *rejoin_out,
                             uint64_t *lost_out, uint64_t *ahead_out, uint64_t *gap_ahead_out, uint64_t *gap_behind_out)
{
    const auto kernel = state ? &mcgp::race_window_kernel<true> : &mcgp::race_window_kernel<false>;
    uint32_t L = 0, lap0 = 0, rows = 0;                         // laps lap0 + 1 .. L are recorded
    const uint32_t B = n_edges + 1, W = n_windows;
    double edge_table[mcgp::kGapEdgeSlots];                     // the call's edges, then +inf (gaps.hip.h: gap_bin)
    uint8_t driver_table[mcgp::kWindowSlots] = {};              // the call's windows, then (driver 0, loss 0): whole groups
    double loss_table[mcgp::kWindowSlots] = {};
    size_t count_lds = 0;
    uint8_t *d_stage;
    const double *d_edges, *d_losses;
    const uint8_t *d_drivers;
    AnalysisKind k = {"pit windows run", "pit windows", "mcgp::race_window_kernel", reinterpret_cast<KernelFn>(kernel),
                      kWindowStageBytes, "rejoin_out", rejoin_out};
    k.check_args = [&]() -> int {
        const int rc = check_gap_edges(n_edges, edges);
        if (rc != MCGP_OK) return rc;
        if (W < 1 || W > mcgp::kMaxPitWindows) return fail(MCGP_E_BAD_ARG, "n_windows must be in [1, 64]");
        if (!window_drivers) return fail(MCGP_E_BAD_ARG, "window_drivers is NULL");
        if (!window_losses) return fail(MCGP_E_BAD_ARG, "window_losses is NULL");
        if (!lost_out) return fail(MCGP_E_BAD_ARG, "lost_out is NULL");
        if (!ahead_out) return fail(MCGP_E_BAD_ARG, "ahead_out is NULL");
        if (!gap_ahead_out) return fail(MCGP_E_BAD_ARG, "gap_ahead_out is NULL");
        if (!gap_behind_out) return fail(MCGP_E_BAD_ARG, "gap_behind_out is NULL");
        for (uint32_t w = 0; w < W; ++w)
            if (!std::isfinite(window_losses[w]) || !(window_losses[w] >= 0.0))
                return fail(MCGP_E_BAD_ARG, "window_losses[" + std::to_string(w) + "] must be finite and >= 0");
        return MCGP_OK;
    };
    k.check_fields = [&]() -> int {
        for (uint32_t w = 0; w < W; ++w)
            if (window_drivers[w] >= n)
                return fail(MCGP_E_BAD_ARG, "window_drivers[" + std::to_string(w) + "]: driver index must be below n");
        return MCGP_OK;
    };
    k.plan = [&](uint32_t laps, uint32_t lap) {
        L = laps, lap0 = lap, rows = (L - lap0) * W * mcgp::kWindowRows;
        fill_edge_table(edge_table, n_edges, edges);
        for (uint32_t w = 0; w < W; ++w) driver_table[w] = window_drivers[w], loss_table[w] = window_losses[w];
        // the counting kernel's columns: 4 x 256 bytes per value, up to 65 values (the gap rows at 63 edges)
        count_lds = (size_t)std::max(n + 2, B + 1) * mcgp::kGapsCountBlock * 4;
        // hist [n][n] | rejoin, lost [L][W][n + 1] | ahead [L][W][n + 2] | gap_ahead, gap_behind [L][W][B + 1].  A race
        // resumed after its last lap records nothing: one row's worth of staging keeps the sizes non-zero
        const size_t cells = (size_t)L * W;
        return AnalysisPlan{{{hist_out, (size_t)n * n}, {rejoin_out, cells * (n + 1)}, {lost_out, cells * (n + 1)},
                             {ahead_out, cells * (n + 2)}, {gap_ahead_out, cells * (B + 1)}, {gap_behind_out, cells * (B + 1)}},
                            std::max<uint64_t>(rows, 1), count_lds, reinterpret_cast<const void *>(&mcgp::window_count_rows)};
    };
    // staging of one chunk in rows of `stride` bytes | edges | window drivers | window losses
    k.regions = [&](Layout &ws, uint64_t stride) {
        ws.add(&d_stage, (size_t)std::max<uint32_t>(rows, 1) * stride);
        ws.add(&d_edges, mcgp::kGapEdgeSlots, edge_table);
        ws.add(&d_losses, mcgp::kWindowSlots, loss_table);
        ws.add(&d_drivers, mcgp::kWindowSlots, driver_table);
    };
    k.launch = [&](const AnalysisChunk &a) -> int {
        hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(a.block), a.lds, nullptr, a.kp, a.st, d_edges, n_edges, d_drivers, d_losses,
                           W, a.m, a.first_sim, a.seed_lo, a.seed_hi, a.count(0), d_stage, a.stride, a.n_batches);
        HIP_TRY(hipGetLastError());
        if (rows) {
            hipLaunchKernelGGL(mcgp::window_count_rows, dim3((uint32_t)std::min<uint64_t>(rows, a.grid_cap)),
                               dim3(mcgp::kGapsCountBlock), count_lds, nullptr, d_stage, a.stride, a.m, rows, n, W, B, lap0,
                               a.count(1), a.count(2), a.count(3), a.count(4), a.count(5));
            HIP_TRY(hipGetLastError());
        }
        return MCGP_OK;
    };
    return run_analysis(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, k);
}

static_assert(sizeof(mcgp::CondAtom) == sizeof(mcgp_condition_atom) && sizeof(mcgp::Cond) == sizeof(mcgp_condition) &&
                  offsetof(mcgp::Cond, atom) == offsetof(mcgp_condition, atom),
              "the device's condition table is the C ABI's array as it is");
static_assert(mcgp::kMaxConditions == MCGP_MAX_CONDITIONS && mcgp::kMaxConditionAtoms == MCGP_MAX_CONDITION_ATOMS &&
                  mcgp::kFactCount == MCGP_FACT_VSCS + 1, "conditions.hip.h and mcgp.h state the same limits");

int32_t mcgp_run_conditions(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                            const mcgp_race_state *state, uint32_t n, uint32_t n_conditions,
                            const mcgp_condition *conditions, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                            int32_t device, uint64_t *hist_out, uint64_t *count_out, uint64_t *cond_hist_out)
{
    const auto kernel = state ? &mcgp::race_conditions_kernel<true> : &mcgp::race_conditions_kernel<false>;
    const uint32_t C = n_conditions;
    uint8_t *d_stage;
    const mcgp::Cond *d_cond;
    AnalysisKind k = {"conditions run", "conditions", "mcgp::race_conditions_kernel", reinterpret_cast<KernelFn>(kernel),
                      kConditionsStageBytes, "count_out", count_out};
    k.check_args = [&]() -> int {
        if (C < 1 || C > mcgp::kMaxConditions) return fail(MCGP_E_BAD_ARG, "n_conditions must be in [1, 64]");
        if (!conditions) return fail(MCGP_E_BAD_ARG, "conditions is NULL");
        return MCGP_OK;
    };
    k.check_fields = [&]() -> int {
        for (uint32_t ci = 0; ci < C; ++ci) {
            const mcgp_condition &cond = conditions[ci];
            const std::string where = "conditions[" + std::to_string(ci) + "]";
            if (cond.n_atoms > mcgp::kMaxConditionAtoms) return fail(MCGP_E_BAD_ARG, where + ".n_atoms must be in [0, 8]");
            for (uint32_t j = 0; j < cond.n_atoms; ++j) {
                const mcgp_condition_atom &at = cond.atom[j];
                const std::string atom = where + ".atom[" + std::to_string(j) + "]";
                if (at.fact < 0 || at.fact >= mcgp::kFactCount)
                    return fail(MCGP_E_BAD_ARG, atom + ".fact: unknown fact " + std::to_string(at.fact));
                const bool per_driver = at.fact <= MCGP_FACT_GAINED;
                if (per_driver && (at.a < 0 || at.a >= (int32_t)n))
                    return fail(MCGP_E_BAD_ARG, atom + ".a: driver index must be in [0, n)");
                if (at.fact == MCGP_FACT_AHEAD_BY) {
                    if (at.b < 0 || at.b >= (int32_t)n) return fail(MCGP_E_BAD_ARG, atom + ".b: driver index must be in [0, n)");
                    if (at.a == at.b) return fail(MCGP_E_BAD_ARG, atom + ".b: AHEAD_BY needs two different drivers");
                }
                if (at.lo > at.hi) return fail(MCGP_E_BAD_ARG, atom + ".lo must not be above .hi");
            }
        }
        return MCGP_OK;
    };
    // hist [n][n] | count [C] | cond_hist [C][n][n]; per simulation the finishing order and one u64 mask
    k.plan = [&](uint32_t, uint32_t) {
        return AnalysisPlan{{{hist_out, (size_t)n * n}, {count_out, C}, {cond_hist_out, cond_hist_out ? (size_t)C * n * n : 0}},
                            (uint64_t)n + 8};
    };
    // staging of one chunk, n rows of `stride` bytes then `stride` u64 masks | condition table
    k.regions = [&](Layout &ws, uint64_t stride) {
        ws.add(&d_stage, (size_t)(n + 8) * stride);
        ws.add(&d_cond, C, reinterpret_cast<const mcgp::Cond *>(conditions));
    };
    k.launch = [&](const AnalysisChunk &a) -> int {
        hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(a.block), a.lds, nullptr, a.kp, a.st, d_cond, C, a.m, a.first_sim,
                           a.seed_lo, a.seed_hi, a.count(0), d_stage, a.stride, a.n_batches);
        HIP_TRY(hipGetLastError());
        const uint32_t groups = (C + mcgp::kCondGroup - 1) / mcgp::kCondGroup;
        hipLaunchKernelGGL(mcgp::conditions_count, dim3(count_grid_x(a.m, mcgp::kCondCountBlock, a.grid_cap, groups), groups),
                           dim3(mcgp::kCondCountBlock), 0, nullptr, d_stage, a.stride, a.m, n, C, a.count(1), a.wanted(2));
        HIP_TRY(hipGetLastError());
        return MCGP_OK;
    };
    return run_analysis(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, k);
}

static_assert(mcgp::kStintStops == MCGP_STINT_STOPS && mcgp::kStintSeq == MCGP_STINT_SEQ &&
                  mcgp::kStintSeqCodes == MCGP_STINT_SEQ_CODES, "stints.hip.h and mcgp.h state the same limits");

int32_t mcgp_run_stints(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        const mcgp_race_state *state, uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                        int32_t device, uint64_t *hist_out, uint64_t *stop_lap_out, uint64_t *stops_pos_out,
                        uint64_t *seq_out)
{
    const auto kernel = state ? &mcgp::race_stints_kernel<true> : &mcgp::race_stints_kernel<false>;
    uint32_t L = 0;
    size_t count_lds = 0;
    uint64_t *d_rec;
    uint8_t *d_pos;
    AnalysisKind k = {"stints run", "stints", "mcgp::race_stints_kernel", reinterpret_cast<KernelFn>(kernel), kStintsStageBytes,
                      "stop_lap_out", stop_lap_out};
    k.plan = [&](uint32_t laps, uint32_t) {
        L = laps;
        // the counting kernel's histograms: 6.4 KiB at 60 laps and 20 cars, 21 KiB at 1000 laps
        count_lds = ((size_t)mcgp::kStintStops * (L + 1) + (size_t)(mcgp::kStintStops + 1) * n + mcgp::kStintSeqCodes) * 4;
        // hist [n][n] | stop_lap [n][4][L + 1] | stops_pos [n][5][n] | seq [n][1296]; per driver and simulation one u64
        // record and one position byte
        return AnalysisPlan{{{hist_out, (size_t)n * n},
                             {stop_lap_out, (size_t)n * mcgp::kStintStops * (L + 1)},
                             {stops_pos_out, stops_pos_out ? (size_t)n * (mcgp::kStintStops + 1) * n : 0},
                             {seq_out, seq_out ? (size_t)n * mcgp::kStintSeqCodes : 0}},
                            9ull * n, count_lds};
    };
    // staging of one chunk, n rows of `stride` u64 records then n rows of `stride` position bytes
    k.regions = [&](Layout &ws, uint64_t stride) {
        ws.add(&d_rec, (size_t)n * stride);
        ws.add(&d_pos, (size_t)n * stride);
    };
    k.launch = [&](const AnalysisChunk &a) -> int {
        hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(a.block), a.lds, nullptr, a.kp, a.st, a.m, a.first_sim, a.seed_lo,
                           a.seed_hi, a.count(0), d_rec, d_pos, a.stride, a.n_batches);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(mcgp::stints_count, dim3(count_grid_x(a.m, mcgp::kStintsCountBlock, a.grid_cap, n), n),
                           dim3(mcgp::kStintsCountBlock), count_lds, nullptr, d_rec, d_pos, a.stride, a.m, n, L, a.count(1),
                           a.wanted(2), a.wanted(3));
        HIP_TRY(hipGetLastError());
        return MCGP_OK;
    };
    return run_analysis(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, k);
}

static_assert(mcgp::kMoveDriverCap == MCGP_MOVE_DRIVER_CAP && mcgp::kMoveRaceCap == MCGP_MOVE_RACE_CAP,
              "moves.hip.h and mcgp.h state the same caps");

int32_t mcgp_run_moves(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                       const mcgp_race_state *state, uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                       int32_t device, uint64_t *hist_out, uint64_t *grid_fin_out, uint64_t *start_gain_out,
                       uint64_t *passes_out, uint64_t *race_passes_out, uint64_t *lap_passes_out,
                       uint64_t *pair_passes_out)
{
    const auto kernel = state ? &mcgp::race_moves_kernel<true> : &mcgp::race_moves_kernel<false>;
    const bool walk = passes_out || race_passes_out || lap_passes_out || pair_passes_out;
    uint32_t L = 0, lap0 = 0;                                   // lap0: the baseline row
    uint64_t rows = 0;
    size_t laps_lds = 0;
    uint8_t *d_stage;
    uint32_t *d_tot;
    AnalysisKind k = {"moves run", "moves", "mcgp::race_moves_kernel", reinterpret_cast<KernelFn>(kernel), kMovesStageBytes,
                      "grid_fin_out", grid_fin_out};
    k.check_args = [&]() -> int {
        if (state && start_gain_out)
            return fail(MCGP_E_BAD_ARG, "start_gain_out must be NULL when a state is given (a start gain is from the grid)");
        return MCGP_OK;
    };
    k.plan = [&](uint32_t laps, uint32_t lap) {
        L = laps, lap0 = state ? lap : 1u, rows = ((uint64_t)L + 2) * n;
        // moves_count_laps' tables and sums: 29 KiB at 60 laps and 20 cars, 52 KiB at 1000 laps and 32 cars
        laps_lds = 9 * (size_t)n * mcgp::kMovesLapsBlock + ((size_t)n * n + 2 * (size_t)(L + 1) + mcgp::kMoveRaceCap + 1) * 4;
        // hist [n][n] | grid_fin [n][n][n] | start_gain [n][2n] | passes [n][4][128] | race_passes [1024] |
        // lap_passes [L + 1][2] | pair_passes [n][n]: the optional ones take no cells when they are not wanted
        return AnalysisPlan{{{hist_out, (size_t)n * n},
                             {grid_fin_out, (size_t)n * n * n},
                             {start_gain_out, start_gain_out ? (size_t)n * 2 * n : 0},
                             {passes_out, passes_out ? (size_t)n * 4 * (mcgp::kMoveDriverCap + 1) : 0},
                             {race_passes_out, race_passes_out ? (size_t)mcgp::kMoveRaceCap + 1 : 0},
                             {lap_passes_out, lap_passes_out ? 2 * (size_t)(L + 1) : 0},
                             {pair_passes_out, pair_passes_out ? (size_t)n * n : 0}},
                            rows, laps_lds};
    };
    // staging of one chunk, (L + 2) n rows of `stride` bytes | every car's packed pass counts, n rows of `stride` u32
    // (only if passes_out)
    k.regions = [&](Layout &ws, uint64_t stride) {
        ws.add(&d_stage, (size_t)rows * stride);
        ws.add(&d_tot, passes_out ? (size_t)n * stride : 0);
    };
    k.launch = [&](const AnalysisChunk &a) -> int {
        uint32_t *tot = passes_out ? d_tot : nullptr;
        hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(a.block), a.lds, nullptr, a.kp, a.st, a.m, a.first_sim, a.seed_lo,
                           a.seed_hi, a.count(0), d_stage, a.stride, a.n_batches);
        HIP_TRY(hipGetLastError());
        if (walk) {
            // a block takes at most kMovesBlockShare simulations, so that its u32 sums cannot wrap (moves.hip.h)
            const uint64_t tiles = (a.m + mcgp::kMovesLapsBlock - 1) / mcgp::kMovesLapsBlock;
            const uint64_t per_block = mcgp::kMovesBlockShare / mcgp::kMovesLapsBlock;
            const uint64_t gx = std::min<uint64_t>(tiles, std::max<uint64_t>(a.grid_cap, (tiles + per_block - 1) / per_block));
            hipLaunchKernelGGL(mcgp::moves_count_laps, dim3((uint32_t)gx), dim3(mcgp::kMovesLapsBlock), laps_lds, nullptr,
                               d_stage, a.stride, a.m, n, L, lap0, tot, a.wanted(4), a.wanted(5), a.wanted(6));
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(mcgp::moves_count_drivers, dim3(count_grid_x(a.m, mcgp::kMovesDriversBlock, a.grid_cap, n), n),
                           dim3(mcgp::kMovesDriversBlock), 0, nullptr, d_stage, tot, a.stride, a.m, n, L, a.count(1),
                           a.wanted(2), a.wanted(3));
        HIP_TRY(hipGetLastError());
        return MCGP_OK;
    };
    return run_analysis(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, k);
}

int32_t mcgp_last_kernel_ms(int32_t device, float *ms_out)
{
    if (!ms_out) return fail(MCGP_E_BAD_ARG, "ms_out is NULL");
    if (device < 0 || device >= kMaxDevices) return fail(MCGP_E_BAD_ARG, "device index out of range");
    DeviceCtx &c = g_ctx[device];
    std::lock_guard<std::mutex> lock(c.mu);
    if (!c.ready || (c.last_timer < 0 && c.last_timer != kCallTimer))
        return fail(MCGP_E_BAD_ARG, "no kernel launched on this device yet");
    HIP_TRY(hipSetDevice(device));
    if (c.last_timer == kCallTimer) {                   // a call of several kernels: everything it ran on the device
        HIP_TRY(hipEventSynchronize(c.call_stop));
        HIP_TRY(hipEventElapsedTime(ms_out, c.call_start, c.call_stop));
        return MCGP_OK;
    }
    HIP_TRY(hipEventSynchronize(c.timer[c.last_timer].stop));
    HIP_TRY(hipEventElapsedTime(ms_out, c.timer[c.last_timer].start, c.timer[c.last_timer].stop));
    return MCGP_OK;
}

int32_t mcgp_stream_kernel_ms(int32_t device, void *stream, float *ms_out)
{
    if (!ms_out) return fail(MCGP_E_BAD_ARG, "ms_out is NULL");
    if (device < 0 || device >= kMaxDevices) return fail(MCGP_E_BAD_ARG, "device index out of range");
    DeviceCtx &c = g_ctx[device];
    std::lock_guard<std::mutex> lock(c.mu);
    if (!c.ready) return fail(MCGP_E_BAD_ARG, "no kernel launched on this device yet");
    for (auto &t : c.timer)
        if (t.used && t.stream == (hipStream_t)stream) {
            HIP_TRY(hipSetDevice(device));
            HIP_TRY(hipEventSynchronize(t.stop));
            HIP_TRY(hipEventElapsedTime(ms_out, t.start, t.stop));
            return MCGP_OK;
        }
    return fail(MCGP_E_BAD_ARG, "no timed launch on this stream (or its entry was recycled by 8 newer streams)");
}

const char *mcgp_last_kernel_name(int32_t device)
{
    if (device < 0 || device >= kMaxDevices || !g_ctx[device].ready) return "";
    return g_ctx[device].last_kernel;
}

int32_t mcgp_last_launch_info(int32_t device, uint32_t *grid_blocks, uint32_t *block_threads, uint32_t *lds_bytes)
{
    if (device < 0 || device >= kMaxDevices || !g_ctx[device].ready ||
        (g_ctx[device].last_timer < 0 && g_ctx[device].last_timer != kCallTimer))
        return fail(MCGP_E_BAD_ARG, "no kernel launched on this device yet");
    if (grid_blocks) *grid_blocks = g_ctx[device].last_grid;
    if (block_threads) *block_threads = g_ctx[device].last_block;
    if (lds_bytes) *lds_bytes = g_ctx[device].last_lds;
    return MCGP_OK;
}

}  // extern "C"
