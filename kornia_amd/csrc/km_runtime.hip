// kornia_amd - C-ABI runtime glue: error reporting, version, device query.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string.h>

#include <atomic>
#include <mutex>

#include "km_common.h"

static thread_local char g_km_error[512] = "";

void km_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_km_error, sizeof(g_km_error), fmt, ap);
    va_end(ap);
}

// ---- launch policy ---------------------------------------------------------------------------------------------------------------
// THE list of the A/B switches: one row per entry of KmConfig - the key km_config_set / km_config_get take, the member, the environment
// variable and how its value is decoded (only the FIRST CHARACTER of a spelling is looked at; v == nullptr: the variable is not set).
// The environment is read ONCE, when the library is first used; launchers read the struct, never the environment.  km_config_set
// changes an entry explicitly (tests, A/B timing of one process) - it is not meant to race with launches - and stores any int: an
// entry that its launcher tests against listed values treats the others as the comment of its decoder says.
// km_warp2d_pair_fwd without KM_PAIR_ALGO: 1 one launch (km_warp_pair_kernel), 0 two launches, 2 one launch for perspective / two for
// affine (what measured faster on each: profiles/README.md, r07)
static const int KM_PAIR_FUSED_DEFAULT = 2;
template <char C>
static int km_dec_is(const char* v) { return v && v[0] == C; }  // 1 for the spelling that starts with C, 0 otherwise and when unset
static int km_dec_warp_fwd(const char* v) {  // generic -> 1, box -> 3 (km_warp_fwd_box_kernel), rows -> 4 (the gather kernel); 0: by the launcher's own rules
    return !v ? 0 : (v[0] == 'g' ? 1 : (v[0] == 'b' ? 3 : (v[0] == 'r' ? 4 : 0)));
}
static int km_dec_warp_gm(const char* v) {  // generic -> 1 (inside the atomic-scatter kernel), rows -> 3 (the gather kernel where the box form would run);
    return !v ? 0 : (v[0] == 'g' ? 1 : (v[0] == 'r' ? 3 : 0));  // 0: the box form where it applies.  Any other non-zero value set by key acts like 3.
}
static int km_dec_not_0(const char* v) { return km_dec_is<'0'>(v) ? 0 : 1; }  // on unless the value starts with 0
static int km_dec_int(const char* v) { return v ? atoi(v) : 0; }
static int km_dec_pair(const char* v) {  // fused -> 1, two -> 0
    return !v ? KM_PAIR_FUSED_DEFAULT : (v[0] == 'f' ? 1 : (v[0] == 't' ? 0 : KM_PAIR_FUSED_DEFAULT));
}
static const struct KmSwitch {
    const char* key;
    int KmConfig::*field;
    const char* env;
    int (*decode)(const char* v);
} g_km_switches[] = {
    {"traversal_fixed", &KmConfig::traversal_fixed, "KM_TRAVERSAL", km_dec_is<'f'>},          // =fixed: every launch walks the batch forward (km_traversal_next)
    {"warp_fwd_algo", &KmConfig::warp_fwd_algo, "KM_WARP_FWD_ALGO", km_dec_warp_fwd},
    {"warp_gm_algo", &KmConfig::warp_gm_algo, "KM_WARP_GM_ALGO", km_dec_warp_gm},
    {"warp_bwd_generic", &KmConfig::warp_bwd_generic, "KM_WARP_BWD_ALGO", km_dec_is<'g'>},    // =generic: the atomic-scatter backward
    {"warp_bwd_fused", &KmConfig::warp_bwd_fused, "KM_WARP_BWD_FUSED", km_dec_not_0},         // =0: the one-read backward off (two launches)
    {"sep_lds", &KmConfig::sep_lds, "KM_SEP_ALGO", km_dec_is<'l'>},                           // =lds: the generic and LDS-tiled filter kernels where a register-tiled one would run
    {"sg_generic", &KmConfig::sg_generic, "KM_SG_ALGO", km_dec_is<'g'>},                      // =generic: the generic spatial-gradient kernel
    {"blur_rows", &KmConfig::blur_rows, "KM_BLUR_ROWS", km_dec_int},                          // =8 / 16 / 32 rows per strip; 0: km_blur_rows chooses
    {"warp_bwd_no_scan", &KmConfig::warp_bwd_no_scan, "KM_WARP_BWD_SCAN", km_dec_is<'0'>},    // =0: no scan for non-finite gradients at pixels that sample outside the source
    {"pair_fused", &KmConfig::pair_fused, "KM_PAIR_ALGO", km_dec_pair},
};
static KmConfig g_km_config;
static std::once_flag g_km_config_once;
static void km_config_init() {
    for (const KmSwitch& sw : g_km_switches) g_km_config.*sw.field = sw.decode(getenv(sw.env));
}
const KmConfig& km_config() {
    std::call_once(g_km_config_once, km_config_init);
    return g_km_config;
}

// Direction of the next launch of a streaming kernel ON THIS STREAM: the parity is per (device, stream), so what another thread,
// stream or device launches never changes the order a stream's own kernels see (re-entrant: the table is lock-free, an entry is
// claimed once and then only touched through its own atomic counter).  Beyond KM_STREAM_SLOTS live streams the direction stays fixed.
#define KM_STREAM_SLOTS 256
static std::atomic<uint64_t> g_km_stream_key[KM_STREAM_SLOTS];  // 0 = free
static std::atomic<uint32_t> g_km_stream_parity[KM_STREAM_SLOTS];
uint32_t km_traversal_next(hipStream_t s) {
    if (km_config().traversal_fixed) return 0u;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t key = ((uint64_t)(uintptr_t)s) ^ ((uint64_t)(dev + 1) << 56) ^ 0x8000000000000000ull;  // never 0
    uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 56);
    for (int probe = 0; probe < KM_STREAM_SLOTS; ++probe, h = (h + 1u) % KM_STREAM_SLOTS) {
        uint64_t k = g_km_stream_key[h].load(std::memory_order_acquire);
        if (k == 0) {
            uint64_t expect = 0;
            if (g_km_stream_key[h].compare_exchange_strong(expect, key, std::memory_order_acq_rel)) k = key;
            else k = expect;
        }
        if (k == key) return g_km_stream_parity[h].fetch_add(1u, std::memory_order_relaxed) & 1u;
    }
    return 0u;
}

// compute units of the current device (cached per device ordinal; 0 on the host build of the kernels)
int km_device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
        v = p.multiProcessorCount > 0 ? p.multiProcessorCount : -1;
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v > 0 ? v : 0;
}

// ---- a forked side stream per device ---------------------------------------------------------------------------------------------------
// km_side_fork(s): work launched on the returned stream starts after everything already queued on `s` and runs BESIDE what `s` is given next;
// km_side_join(s) makes `s` wait for it.  One non-blocking stream and two events per device, created on first use; the record / wait pairs of
// concurrent host threads are serialised by a mutex (a later thread's record only ever makes an earlier thread's wait cover more).  Returns
// nullptr - the caller then launches on `s` itself - while `s` is being captured into a graph, on the host build of the kernels (no device)
// and when a stream or an event cannot be created.
struct KmSide {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int state = 0;  // 0 untried, 1 ready, -1 unavailable
    std::mutex mu;
};
static KmSide g_km_side[64];
hipStream_t km_side_fork(hipStream_t s) {
    int dev = 0;
    if (km_device_cus() <= 0 || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;
    }
    KmSide& k = g_km_side[dev];
    std::lock_guard<std::mutex> lock(k.mu);
    if (k.state == 0) {
        k.state = (hipStreamCreateWithFlags(&k.stream, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&k.fork, hipEventDisableTiming) == hipSuccess &&
                   hipEventCreateWithFlags(&k.join, hipEventDisableTiming) == hipSuccess) ? 1 : -1;
        if (k.state < 0) (void)hipGetLastError();
    }
    if (k.state < 0) return nullptr;
    if (hipEventRecord(k.fork, s) != hipSuccess || hipStreamWaitEvent(k.stream, k.fork, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return k.stream;
}
// after the side stream's work has been launched: `s` waits for it
int km_side_join(hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    KmSide& k = g_km_side[dev];
    std::lock_guard<std::mutex> lock(k.mu);
    if (k.state != 1) return -1;
    hipError_t e = hipEventRecord(k.join, k.stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, k.join, 0);
    if (e != hipSuccess) { km_set_error("km_side_join: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

int km_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        km_set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// ---- km_stream_copy: the copy the hot kernels are compared with (bench.py: roofline.measured_streaming_copy_GBps) --------------------
// ONE 16-byte piece per thread, one workgroup per 4 KB, no loop: the shape that streams fastest on this part (profiles/r02_hbm_shapes.txt: 6.2 TB/s;
// two / four / eight pieces per thread 5.8 / 5.7 / 4.3, a grid-stride loop over ~8 resident workgroups per CU 5.2 - round 6, run 3)
template <bool NT>
__global__ __launch_bounds__(256) void km_stream_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n16) {
    typedef float km_f4v __attribute__((ext_vector_type(4)));
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n16) {
        if (NT) {
            const km_f4v v = __builtin_nontemporal_load(reinterpret_cast<const km_f4v*>(src) + i);
            __builtin_nontemporal_store(v, reinterpret_cast<km_f4v*>(dst) + i);
        } else {
            dst[i] = src[i];
        }
    }
}

extern "C" {

int km_abi_version(void) { return KM_ABI_VERSION; }

// entry points added after set 3, one bit per group (include/kornia_amd.h, Versioning)
int km_abi_features(void) { return KM_ABI_FEATURES; }

int km_stream_copy(const void* src, void* dst, long long bytes, int nontemporal, void* stream) {
    KM_REQUIRE(bytes >= 0 && bytes % 16 == 0, "km_stream_copy: bytes must be a non-negative multiple of 16");
    if (bytes == 0) return 0;
    KM_REQUIRE(src && dst && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "km_stream_copy: null or unaligned pointer");
    const size_t n16 = (size_t)bytes / 16;
    const size_t blocks = (n16 + 255) / 256;
    KM_REQUIRE(blocks < (1ull << 31), "km_stream_copy: at most 8 TiB per call");
    hipStream_t s = (hipStream_t)stream;
    if (nontemporal) hipLaunchKernelGGL((km_stream_copy_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)src, (float4*)dst, n16);
    else hipLaunchKernelGGL((km_stream_copy_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)src, (float4*)dst, n16);
    return km_check_launch("km_stream_copy");
}

int km_set_traversal(int mode) {
    (void)km_config();
    const int prev = g_km_config.traversal_fixed;
    g_km_config.traversal_fixed = mode ? 1 : 0;
    return prev;
}

// Explicit setter of a launch-policy entry (the keys of g_km_switches); returns the previous value, -1 for an unknown key.
// For tests and A/B timing: call it between launches, not concurrently with them.
static int* km_config_field(const char* key) {
    if (key)
        for (const KmSwitch& sw : g_km_switches)
            if (strcmp(sw.key, key) == 0) return &(g_km_config.*sw.field);
    return nullptr;
}
int km_config_set(const char* key, int value) {
    (void)km_config();
    int* f = km_config_field(key);
    if (!f) { km_set_error("km_config_set: unknown key '%s'", key ? key : "(null)"); return -1; }
    const int prev = *f;
    *f = value;
    return prev;
}
// current value of a launch-policy entry (-1: unknown key)
int km_config_get(const char* key) {
    (void)km_config();
    const int* f = km_config_field(key);
    if (!f) { km_set_error("km_config_get: unknown key '%s'", key ? key : "(null)"); return -1; }
    return *f;
}

const char* km_last_error(void) { return g_km_error; }

// Fills name (up to n bytes) with the gcnArchName of the current device; returns CU count or <0.
int km_device_info(char* name, int n) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        km_set_error("hipGetDevice: %s", hipGetErrorString(e));
        return -1;
    }
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) {
        km_set_error("hipGetDeviceProperties: %s", hipGetErrorString(e));
        return -1;
    }
    if (name && n > 0) snprintf(name, (size_t)n, "%s", p.gcnArchName);
    return p.multiProcessorCount;
}

}  // extern "C"
