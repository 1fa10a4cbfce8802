// How a headline sweep of scan_ring_kernel spends its time per workgroup: start, first stage landed, last stage issued, end and
// the CU of every workgroup (wall_clock64), from the measurement-only build of nmn_scan_ring.hip (NMN_RING_WG_CLOCK).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o ring_clock ring_clock.hip && ./ring_clock [rows] [ld] [grid ...]
// grid: 0 = one workgroup per wmax group (NMN_NO_RING_EVEN); M:T = M + T chunks per CU, the last T of them short, one workgroup per
// CU taking them from the ticket counter (ring_set_grid); there a workgroup's drain is that of its last chunk (start-up: read grid 0).
// Reports per launch configuration: kernel time (events), how long fewer than all CUs hold a workgroup at the start (ramp) and
// at the end (ragged end), the idle CU time over the sweep as a fraction of it, and per-workgroup start-up and drain times.
#define NMN_RING_WG_CLOCK 1
#include "../../neumann_amd/csrc/nmn_scan_ring.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace nmn;

__global__ void fill_rows(float* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = i * 0x9E3779B97F4A7C15ull + 0x1234567;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 32;
        p[i] = (float)(int)(x & 0xFFFF) * (1.0f / 32768.0f) - 1.0f;
    }
}

__global__ void fill_const(float* p, size_t n, float v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

static double pct(std::vector<double> v, double q) {
    std::sort(v.begin(), v.end());
    return v[(size_t)std::min<double>(v.size() - 1, q * (v.size() - 1) + 0.5)];
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    const uint32_t ld = argc > 2 ? (uint32_t)atoi(argv[2]) : 768;
    std::vector<std::pair<uint32_t, uint32_t>> cfgs;  // (workgroups per CU: long, short)
    for (int i = 3; i < argc; i++) {
        unsigned m = 0, t = 0;
        sscanf(argv[i], "%u:%u", &m, &t);
        cfgs.push_back({m, t});
    }
    if (cfgs.empty()) cfgs.push_back({0, 0});
    const uint32_t n_tiles = (uint32_t)((rows + kTileRows - 1) / kTileRows);
    int clk_khz = 0;
    CK(hipDeviceGetAttribute(&clk_khz, hipDeviceAttributeWallClockRate, 0));
    int n_cu = 0;
    CK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, 0));
    float *corpus, *norms, *qpad;
    QInfo* qinfo;
    uint32_t *scores, *tmax, *wmax;
    unsigned long long* clk;
    uint32_t* ctr;
    CK(hipMalloc(&ctr, 8));
    CK(hipMemset(ctr, 0, 8));
    CK(hipMalloc(&corpus, (size_t)n_tiles * kTileRows * ld * 4));
    CK(hipMalloc(&norms, (size_t)n_tiles * kTileRows * 4));
    CK(hipMalloc(&qpad, (size_t)ld * 4));
    CK(hipMalloc(&qinfo, sizeof(QInfo)));
    CK(hipMalloc(&scores, (size_t)n_tiles * kTileRows * 4));
    CK(hipMalloc(&tmax, (size_t)n_tiles * 4));
    CK(hipMalloc(&wmax, (size_t)kMaxScanWaves * 4));
    CK(hipMalloc(&clk, (size_t)n_tiles * 5 * 8));  // (at most one workgroup per tile)
    hipLaunchKernelGGL(fill_rows, dim3(4096), dim3(256), 0, 0, corpus, (size_t)n_tiles * kTileRows * ld);
    hipLaunchKernelGGL(fill_const, dim3(4096), dim3(256), 0, 0, norms, (size_t)n_tiles * kTileRows, 1.0f);
    hipLaunchKernelGGL(fill_rows, dim3(4), dim3(256), 0, 0, qpad, (size_t)ld);
    QInfo qi{};
    qi.qmag = 1.0f;
    CK(hipMemcpy(qinfo, &qi, sizeof qi, hipMemcpyHostToDevice));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(nmn_ring_clk), &clk, sizeof clk));
    CK(hipDeviceSynchronize());
    printf("rows %llu ld %u tiles %u, %d CUs, wall clock %d kHz\n", (unsigned long long)rows, ld, n_tiles, n_cu, clk_khz);

    ScanParams p{};
    p.corpus = corpus;
    p.norms = norms;
    p.qpad = qpad;
    p.qinfo = qinfo;
    p.scores = scores;
    p.tmax = tmax;
    p.wmax = wmax;
    p.n_rows = rows;
    p.ld = ld;
    p.n_tiles = n_tiles;
    p.nq = p.nql = 1;
    p.metric = NMN_METRIC_COSINE;
    p.tiles_per_wave = (n_tiles + kMaxScanWaves - 1) / kMaxScanWaves;
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (auto cfg : cfgs) {
        p.ring_wgs = cfg.first ? (cfg.first + cfg.second) * (uint32_t)n_cu : 0u;  // (ring_set_grid's split with these counts)
        p.ring_tail = cfg.first ? cfg.second * (uint32_t)n_cu : 0u;
        p.ring_grid = (uint32_t)n_cu;
        p.ring_ctr = ctr;
        const uint32_t wgs = p.ring_wgs ? p.ring_grid : (n_tiles + p.tiles_per_wave - 1) / p.tiles_per_wave;
        if (wgs > n_tiles) {
            printf("grid %u:%u: more workgroups than tiles (the clock buffer holds one per tile)\n", cfg.first, cfg.second);
            continue;
        }
        std::vector<float> ms;
        for (int rep = 0; rep < 8; rep++) {
            CK(hipMemsetAsync(wmax, 0, (size_t)kMaxScanWaves * 4, 0));
            CK(hipEventRecord(a, 0));
            CK(launch_scan_ring(p, 0));
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            float t = 0;
            CK(hipEventElapsedTime(&t, a, b));
            if (rep >= 2) ms.push_back(t);
        }
        std::vector<unsigned long long> h((size_t)wgs * 5);
        CK(hipMemcpy(h.data(), clk, h.size() * 8, hipMemcpyDeviceToHost));
        const double us = 1000.0 / clk_khz;  // microseconds per tick
        unsigned long long k0 = ~0ull, k1 = 0;
        for (uint32_t w = 0; w < wgs; w++) {
            k0 = std::min(k0, h[w * 5 + 0]);
            k1 = std::max(k1, h[w * 5 + 3]);
        }
        // busy CUs over time: +1 at a start, -1 at an end
        std::vector<std::pair<unsigned long long, int>> ev;
        for (uint32_t w = 0; w < wgs; w++) {
            ev.push_back({h[w * 5 + 0], +1});
            ev.push_back({h[w * 5 + 3], -1});
        }
        std::sort(ev.begin(), ev.end());
        int busy = 0, peak = 0;
        for (auto& e : ev) peak = std::max(peak, busy += e.second);
        double idle = 0, ramp = -1, tail = 0;
        busy = 0;
        unsigned long long prev = k0, last_full = k0;
        for (auto& e : ev) {
            idle += (double)(peak - busy) * (e.first - prev);
            prev = e.first;
            busy += e.second;
            if (busy == peak) {
                if (ramp < 0) ramp = (e.first - k0) * us;
                last_full = e.first;
            }
        }
        for (auto& e : ev) if (e.first > last_full) { tail = (k1 - last_full) * us; break; }
        std::vector<double> dur, startup, drain;
        std::vector<int> per_cu(65536, 0);
        for (uint32_t w = 0; w < wgs; w++) {
            dur.push_back((h[w * 5 + 3] - h[w * 5 + 0]) * us);
            startup.push_back((h[w * 5 + 1] - h[w * 5 + 0]) * us);
            if (h[w * 5 + 2] >= h[w * 5 + 0]) drain.push_back((h[w * 5 + 3] - h[w * 5 + 2]) * us);
            per_cu[h[w * 5 + 4] & 0xFFFF]++;
        }
        int cu_min = 1 << 30, cu_max = 0;
        for (int c : per_cu) if (c) { cu_min = std::min(cu_min, c); cu_max = std::max(cu_max, c); }
        std::sort(ms.begin(), ms.end());
        const double span = (k1 - k0) * us;
        printf("grid %2u:%-2u -> %4u workgroups: kernel med %.3f ms min %.3f | clock span %.1f us, peak busy %d, ramp to peak %.1f us, "
               "ragged end (fewer than peak busy) %.1f us, idle CU time %.2f %% of span | per workgroup: duration med %.1f p5 %.1f p95 %.1f us, "
               "start-up (first stage landed) med %.2f p95 %.2f us, drain (last issue -> end) med %.2f p95 %.2f us | workgroups per CU id %d..%d\n",
               cfg.first, cfg.second, wgs, ms[ms.size() / 2], ms[0], span, peak, ramp, tail, 100.0 * idle / ((double)peak * (k1 - k0)), pct(dur, 0.5),
               pct(dur, 0.05), pct(dur, 0.95), pct(startup, 0.5), pct(startup, 0.95), drain.empty() ? 0.0 : pct(drain, 0.5),
               drain.empty() ? 0.0 : pct(drain, 0.95), cu_min, cu_max);
    }
    return 0;
}
