// C ABI of libuno_spectral.so (declared in include/uno_spectral.h), the core: version, error record, profiler, the calling thread's
// scratch, the settings + the twiddle-table cache.  The entry points of the kernels are in capi_spectral.hip (transforms, per-mode
// GEMMs, spectral convolutions) and capi_pointwise.hip (resampling, channel mix / weight gradient, lift, projection, GELU forms,
// InstanceNorm, Adam).  Every object below exists ONCE in the library; the other units reach it through uno_common.h.
#include "../../include/uno_spectral.h"
#include "uno_common.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace uno {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// (cos, sin)(2 pi n / N) evaluated in double with the phase reduced in integers, exact at the
// multiples of pi/2 (so that sin(pi l) terms of Nyquist / w = 0 columns vanish identically).
float2 twiddle_value(long long n, int N) {
    const double two_pi = 6.283185307179586476925286766559;
    double c, s;
    const long long n4 = 4LL * n;
    if (n4 % N == 0) {
        switch ((n4 / N) & 3) {
            case 0: c = 1; s = 0; break;
            case 1: c = 0; s = 1; break;
            case 2: c = -1; s = 0; break;
            default: c = 0; s = -1; break;
        }
    } else {
        c = std::cos(two_pi * n / N);
        s = std::sin(two_pi * n / N);
    }
    return make_float2((float)c, (float)s);
}
static void fill_twiddles(int N, std::vector<float2>& t) {
    t.resize(N);
    for (int n = 0; n < N; ++n) t[n] = twiddle_value(n, N);
}

void* upload_table(const void* host, size_t bytes) {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    if (hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) return nullptr;
    void* d = nullptr;
    hipStream_t st = nullptr;
    bool ok = hipMalloc(&d, bytes) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
              hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    if (st) (void)hipStreamDestroy(st);
    if (!ok && d) { (void)hipFree(d); d = nullptr; }
    (void)hipThreadExchangeStreamCaptureMode(&mode);          // back to the caller's mode
    return d;
}

const float2* twiddle_table(int N) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, float2*> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("hipGetDevice failed"); return nullptr; }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({dev, N});
    if (it != cache.end()) return it->second;
    std::vector<float2> host;
    fill_twiddles(N, host);
    float2* d = static_cast<float2*>(upload_table(host.data(), sizeof(float2) * N));
    if (!d) {
        set_error("twiddle table allocation for N=%d failed: %s", N, hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    cache[{dev, N}] = d;
    return d;
}

// ---------------------------------------------------------------------------- profiling
struct ProfRecord { char name[64]; double bytes; hipEvent_t e0, e1; float ms; };
static std::mutex g_prof_mu;
static std::vector<ProfRecord> g_prof;
static int g_prof_cap = 0;
static bool g_prof_on = false;

ProfScope::ProfScope(const char* name, double bytes, hipStream_t s) : slot(-1), stream(s) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof_on || (int)g_prof.size() >= g_prof_cap) return;
    ProfRecord r;
    snprintf(r.name, sizeof(r.name), "%s", name);
    r.bytes = bytes; r.ms = 0.f;
    if (hipEventCreate(&r.e0) != hipSuccess) return;
    if (hipEventCreate(&r.e1) != hipSuccess) { (void)hipEventDestroy(r.e0); return; }
    (void)hipEventRecord(r.e0, s);
    g_prof.push_back(r);
    slot = (int)g_prof.size() - 1;
}

ProfScope::~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (slot < (int)g_prof.size()) (void)hipEventRecord(g_prof[slot].e1, stream);
}

// caller-provided scratch of the calling thread (uno_scratch_provide): the any-mode transforms' intermediate spectrum, K8-S's pre-split weights
static thread_local Scratch t_scratch = {nullptr, 0};
const Scratch& thread_scratch() { return t_scratch; }

static int g_reserved_cus = 0;
int reserved_cus() { return __atomic_load_n(&g_reserved_cus, __ATOMIC_RELAXED); }
static int g_sweep_alternation = 255;
static thread_local unsigned t_sweep_count = 0;
// family bits of the setting: 1 K1, 2 K3, 4 K7, 8 K8, 16 K9, 32 InstanceNorm, 64 GELU-projection backward, 128 lift kernels; a launch of a
// family that is switched off runs front to back and does not advance the counter.  Bit 8 (256 | mask) pins the direction: every launch of a
// masked family runs reversed and the counter is neither read nor advanced (the tests' handle on the direction: a caller cannot see or set
// the counter of another thread, autograd's among them)
int next_sweep_reversed(int family) {
    const int a = __atomic_load_n(&g_sweep_alternation, __ATOMIC_RELAXED);
    if (!(a & family)) return 0;
    if (a & 256) return 1;
    return (int)(t_sweep_count++ & 1u);
}

}  // namespace uno

using namespace uno;

extern "C" {

int uno_abi_version(void) { return UNO_SPECTRAL_ABI_VERSION; }

void* uno_upload_table(const void* host, long long bytes) {
    if (!host || bytes < 1) { set_error("uno_upload_table: bad arguments"); return nullptr; }
    void* d = upload_table(host, (size_t)bytes);
    if (!d) set_error("uno_upload_table: allocation / upload of %lld bytes failed: %s", bytes, hipGetErrorString(hipGetLastError()));
    return d;
}

int uno_sweep_alternation(int enable) {
    return __atomic_exchange_n(&uno::g_sweep_alternation, enable == 1 ? 255 : (enable & (enable < 0 ? 255 : 511)), __ATOMIC_RELAXED);      // (1: all families; other values: a mask, development; 256 | mask: pinned reversed; negative values keep their low eight bits, as before)
}

int uno_reserve_cus(int n) {
    if (n < 0) n = 0;
    return __atomic_exchange_n(&uno::g_reserved_cus, n, __ATOMIC_RELAXED);
}

int uno_profile_begin(int max_records) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    g_prof.clear();
    g_prof_cap = max_records > 0 ? max_records : 0;
    g_prof.reserve(g_prof_cap);
    g_prof_on = g_prof_cap > 0;
    return 0;
}

int uno_profile_end(void) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on = false;
    for (auto& r : g_prof) {
        if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&r.ms, r.e0, r.e1) != hipSuccess) r.ms = -1.f;
    }
    return (int)g_prof.size();
}

int uno_profile_get(int index, char* name, int name_len, double* ms, double* bytes) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (index < 0 || index >= (int)g_prof.size() || !name || name_len < 1 || !ms || !bytes) {
        set_error("uno_profile_get: bad index or null pointer");
        return -1;
    }
    snprintf(name, (size_t)name_len, "%s", g_prof[index].name);
    *ms = g_prof[index].ms;
    *bytes = g_prof[index].bytes;
    return 0;
}

const char* uno_last_error(void) { return g_err; }

int uno_scratch_provide(void* ptr, long long bytes) {
    if (bytes < 0 || (bytes > 0 && !ptr)) { set_error("uno_scratch_provide: bad buffer"); return -1; }
    t_scratch.ptr = bytes > 0 ? ptr : nullptr;
    t_scratch.bytes = bytes > 0 ? (size_t)bytes : 0;
    return 0;
}

}  // extern "C"
