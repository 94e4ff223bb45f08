// Device keep-filter against a plain host pass, for a cloud that starts and
// ends in host memory (development probe; DESIGN.md §5m quotes its output).
// Shadow, f32, 3-D, 3 descriptor rows (the normals), sin(eps = 0.1):
//   - pmx_keep_filter end to end (upload, kernels, download; a host clock
//     around the call, which synchronises before it returns)
//   - the same predicate and compaction as one host thread, same process,
//     alternating with the device call
//   - the upload and the download alone (pageable hipMemcpyAsync + sync, as
//     the library issues them)
// and checks that both paths return the same bytes.
// build: hipcc -O2 -std=c++17 -ffp-contract=off tools/keep_probe.cpp -Iinclude \
//        -Llibpointmatcher_amd/lib -lpmx -Wl,-rpath,'$ORIGIN/../libpointmatcher_amd/lib' -o tools/keep_probe
// run:   tools/keep_probe [points = 1000000] [rounds = 20]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pmx.h"

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define CK(x)                                                          \
    do {                                                               \
        hipError_t e_ = (x);                                           \
        if (e_ != hipSuccess) {                                        \
            std::printf("%s failed: %s\n", #x, hipGetErrorString(e_)); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static void unit(float* v) {
    float z = v[0] * v[0];
    z = z + v[1] * v[1];
    z = z + v[2] * v[2];
    if (z > 0.f) {
        const float s = std::sqrt(z);
        v[0] = v[0] / s;
        v[1] = v[1] / s;
        v[2] = v[2] / s;
    }
}

// Shadow.cpp:62-94 as one host thread: predicate, then the column copies
static int64_t host_shadow(const float* f, const float* d, int64_t n, float sin_eps, float* of, float* od) {
    int64_t j = 0;
    for (int64_t i = 0; i < n; ++i) {
        float nv[3] = {d[i * 3], d[i * 3 + 1], d[i * 3 + 2]};
        float pv[3] = {f[i * 4], f[i * 4 + 1], f[i * 4 + 2]};
        unit(nv);
        unit(pv);
        float dot = nv[0] * pv[0];
        dot = dot + nv[1] * pv[1];
        dot = dot + nv[2] * pv[2];
        const float v = dot < 0.f ? -dot : dot;
        if (v > sin_eps) {
            std::memcpy(of + j * 4, f + i * 4, 16);
            std::memcpy(od + j * 3, d + i * 3, 12);
            ++j;
        }
    }
    return j;
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 1000000;
    const int rounds = argc > 2 ? std::atoi(argv[2]) : 20;
    const float sin_eps = std::sin(0.1f);
    std::vector<float> f((size_t)n * 4), d((size_t)n * 3), of(f.size()), od(d.size()), hf(f.size()), hd(d.size());
    uint64_t s = 88172645463325252ull;
    auto rnd = [&] {  // xorshift64: uniform in [-1, 1)
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (float)((double)(s >> 11) / 4503599627370496.0 - 1.0);
    };
    for (int64_t i = 0; i < n; ++i) {
        for (int r = 0; r < 3; ++r) f[i * 4 + r] = 20.f * rnd();
        f[i * 4 + 3] = 1.f;
        // normals mostly across the line of sight, as on a scanned surface seen head on
        for (int r = 0; r < 3; ++r) d[i * 3 + r] = 0.02f * rnd() + (rnd() > 0.f ? f[i * 4 + r] / 20.f : 0.f);
    }
    int64_t m = 0, hm = 0;
    for (int w = 0; w < 3; ++w)
        if (pmx_keep_filter(0, PMX_F32, f.data(), 4, n, d.data(), 3, PMX_KEEP_SHADOW, 0, 0, sin_eps, of.data(),
                            od.data(), &m)) {
            std::printf("pmx_keep_filter failed: %s\n", pmx_last_error(nullptr));
            return 1;
        }
    std::vector<double> td, th;
    for (int r = 0; r < rounds; ++r) {
        double t = now();
        if (pmx_keep_filter(0, PMX_F32, f.data(), 4, n, d.data(), 3, PMX_KEEP_SHADOW, 0, 0, sin_eps, of.data(),
                            od.data(), &m))
            return 1;
        td.push_back(now() - t);
        t = now();
        hm = host_shadow(f.data(), d.data(), n, sin_eps, hf.data(), hd.data());
        th.push_back(now() - t);
    }
    const bool same = m == hm && !std::memcmp(of.data(), hf.data(), (size_t)m * 16) &&
                      !std::memcmp(od.data(), hd.data(), (size_t)m * 12);
    // the copies alone
    void* dev = nullptr;
    const size_t in_bytes = (size_t)n * 28, out_bytes = (size_t)m * 28;
    CK(hipMalloc(&dev, in_bytes));
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::vector<double> tu, tdn;
    for (int r = 0; r < rounds + 3; ++r) {
        double t = now();
        CK(hipMemcpyAsync(dev, f.data(), (size_t)n * 16, hipMemcpyHostToDevice, st));
        CK(hipMemcpyAsync((char*)dev + (size_t)n * 16, d.data(), (size_t)n * 12, hipMemcpyHostToDevice, st));
        CK(hipStreamSynchronize(st));
        const double u = now() - t;
        t = now();
        CK(hipMemcpyAsync(of.data(), dev, (size_t)m * 16, hipMemcpyDeviceToHost, st));
        CK(hipMemcpyAsync(od.data(), (char*)dev + (size_t)n * 16, (size_t)m * 12, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        if (r >= 3) {
            tu.push_back(u);
            tdn.push_back(now() - t);
        }
    }
    CK(hipFree(dev));
    std::printf("{\"points\": %lld, \"kept\": %lld, \"same_bytes\": %s, \"rounds\": %d, "
                "\"device_call_ms\": {\"median\": %.3f, \"min\": %.3f}, \"host_loop_ms\": {\"median\": %.3f, \"min\": %.3f}, "
                "\"upload_ms\": {\"median\": %.3f, \"bytes\": %zu}, \"download_ms\": {\"median\": %.3f, \"bytes\": %zu}}\n",
                (long long)n, (long long)m, same ? "true" : "false", rounds, 1e3 * median(td),
                1e3 * *std::min_element(td.begin(), td.end()), 1e3 * median(th),
                1e3 * *std::min_element(th.begin(), th.end()), 1e3 * median(tu), in_bytes, 1e3 * median(tdn), out_bytes);
    return same ? 0 : 3;
}
