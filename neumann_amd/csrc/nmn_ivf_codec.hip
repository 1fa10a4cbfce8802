// nmn_ivf_codec.hip — device kernels of the IVF-PQ and IVF-Binary storages (tensor_store/src/ivf.rs:61-157, 222-406;
// pq.rs:114-430; binary_quantization.rs:27-155), bit for bit: built with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt like nmn_exact.hip / nmn_kmeans.hip.
//
// Every quantity the reference computes on these paths is a plain sequential f32 sum, a first minimum, a table lookup or
// an integer popcount, so one thread restates one of them in the reference's order:
//   residual     v - centroid[list(v)], one f32 subtract per element (ivf.rs:238-245, 299-303, 358-362)
//   pq encode    per subspace the first k with `dist < best_dist`, best_dist from f32::MAX, code `k as u8` (pq.rs:203-239)
//   adc table    table[m][k] = sum_d (r_{m,d} - cb_{m,k,d})^2, sequential from -0.0 (pq.rs:268-296, 331-338)
//   adc distance sqrt(sum_m table[m][code_m]), sequential over m; f32::MAX for an empty table (pq.rs:392-413)
//   binary       bit i of word i/64 = v[i] > t (binary_quantization.rs:70-88); hamming as f32 / dim as f32 (128-134)
// The scans write the NEGATED distance of every candidate in candidate order (probe order of the list, then position in
// the list = id order), so the large-k sort (nmn_sortk.hip: score desc, candidate index asc) is exactly the reference's
// stable sort by distance (ivf.rs:402-404) — no margin, no rescore, ties in the key.
#include <algorithm>

#include "nmn_internal.h"

#pragma clang fp contract(off)

namespace nmn {

namespace {

constexpr float kF32Max = 3.402823466e+38f;
constexpr uint32_t kCodecRowsPerBlock = 1024;  // candidate rows per workgroup of a list scan
constexpr size_t kLdsBudget = 64 * 1024;       // LDS a table / codebook may take without raising the kernel's limit

// out[m][i][0 .. subdim) = rows[i][m * subdim ..] - cents[assign[i]][m * subdim ..]: the residuals of n rows split into M
// contiguous n x subdim matrices (each one feeds the exact k-means as an ordinary flat index, and the encoder)
__global__ __launch_bounds__(256) void pq_residual_kernel(const float* __restrict__ rows, uint32_t ld_r, const float* __restrict__ cents,
                                                          uint32_t ld_c, const uint32_t* __restrict__ assign, uint64_t n, uint32_t dim,
                                                          uint32_t subdim, float* __restrict__ out) {
    const uint64_t total = n * dim;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = e / dim;
        const uint32_t j = (uint32_t)(e - i * dim);
        const uint32_t m = j / subdim, d = j - m * subdim;
        const float r = rows[i * ld_r + j] - cents[(uint64_t)assign[i] * ld_c + j];
        out[((uint64_t)m * n + i) * subdim + d] = r;
    }
}

// PQCodebook::encode (pq.rs:203-239): thread = one row of subspace blockIdx.y; the subspace's codebook (K x subdim) in LDS
// when it fits (every lane reads the same codeword element: a broadcast)
template <bool kLds>
__global__ __launch_bounds__(256) void pq_encode_kernel(const float* __restrict__ res, uint64_t n, uint32_t M, uint32_t subdim,
                                                        const float* __restrict__ cb, uint32_t K, uint8_t* __restrict__ codes) {
    extern __shared__ float s_cb[];
    const uint32_t m = blockIdx.y;
    const float* cbm = cb + (uint64_t)m * K * subdim;
    if (kLds) {
        for (uint32_t e = threadIdx.x; e < K * subdim; e += blockDim.x) s_cb[e] = cbm[e];
        __syncthreads();
    }
    const float* book = kLds ? s_cb : cbm;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const float* x = res + ((uint64_t)m * n + i) * subdim;
        uint32_t best_idx = 0;
        float best = kF32Max;
        for (uint32_t k = 0; k < K; k++) {
            const float* y = book + (size_t)k * subdim;
            float dist = -0.0f;  // `.sum()`
            for (uint32_t d = 0; d < subdim; d++) {
                const float t = x[d] - y[d];
                dist = dist + t * t;
            }
            if (dist < best) {  // first minimum; a NaN never wins
                best = dist;
                best_idx = k;
            }
        }
        codes[i * M + m] = (uint8_t)best_idx;  // `k as u8`: wraps when K > 256
    }
}

// one probed list of one query: where its codes are (list-major row), how many, where its candidates go
struct CodecSeg {
    uint32_t list, start, count, cand;
};

// the ADC tables of every (query, probed list) of a group: residual q - centroid[list] in LDS, then
// tables[(q * np + i)][m][k] for k < Kt = min(K, 256) (codes only ever address those)
__global__ __launch_bounds__(256) void pq_table_kernel(const float* __restrict__ queries, uint32_t dim, const float* __restrict__ cents,
                                                       uint32_t ld_c, const CodecSeg* __restrict__ segs, uint32_t np,
                                                       const float* __restrict__ cb, uint32_t K, uint32_t Kt, uint32_t M, uint32_t subdim,
                                                       float* __restrict__ tables) {
    extern __shared__ float s_r[];
    const uint32_t i = blockIdx.x, q = blockIdx.y;
    const CodecSeg sg = segs[(size_t)q * np + i];
    if (sg.count == 0) return;  // (not probed, or an empty list: no candidate reads this table)
    const float* qv = queries + (size_t)q * dim;
    const float* c = cents + (uint64_t)sg.list * ld_c;
    for (uint32_t j = threadIdx.x; j < dim; j += blockDim.x) s_r[j] = qv[j] - c[j];
    __syncthreads();
    float* tab = tables + ((size_t)q * np + i) * M * Kt;
    for (uint32_t e = threadIdx.x; e < M * Kt; e += blockDim.x) {
        const uint32_t m = e / Kt, k = e - m * Kt;
        const float* x = s_r + (size_t)m * subdim;
        const float* y = cb + ((uint64_t)m * K + k) * subdim;
        float dist = -0.0f;
        for (uint32_t d = 0; d < subdim; d++) {
            const float t = x[d] - y[d];
            dist = dist + t * t;
        }
        tab[e] = dist;
    }
}

// ADCTable::distance for the rows of one probed list (blockIdx.x), a chunk of them (blockIdx.y), one query (blockIdx.z):
// the table in LDS when it fits, the M codes of a row read 16 bytes at a time when M allows, the sum in m order.
template <bool kLds>
__global__ __launch_bounds__(256) void pq_scan_kernel(const float* __restrict__ tables, const uint8_t* __restrict__ codes, uint32_t M,
                                                      uint32_t Kt, const CodecSeg* __restrict__ segs, uint32_t np,
                                                      const uint64_t* __restrict__ score_base, uint32_t* __restrict__ scores) {
    extern __shared__ float s_t[];
    const uint32_t i = blockIdx.x, q = blockIdx.z;
    const CodecSeg sg = segs[(size_t)q * np + i];
    const uint32_t r0 = blockIdx.y * kCodecRowsPerBlock;
    if (r0 >= sg.count) return;
    const float* gt = tables + ((size_t)q * np + i) * M * Kt;
    if (kLds) {
        for (uint32_t e = threadIdx.x; e < M * Kt; e += blockDim.x) s_t[e] = gt[e];
        __syncthreads();
    }
    const float* tab = kLds ? s_t : gt;
    uint32_t* out = scores + score_base[q] + sg.cand;
    const uint32_t r1 = min(sg.count, r0 + kCodecRowsPerBlock);
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
        const uint8_t* c = codes + (uint64_t)(sg.start + r) * M;
        float sum = -0.0f;  // `.sum()` over m in order
        if (Kt == 0) {
            sum = kF32Max;  // empty table (K' = 0): `f32::MAX`
        } else if ((M & 15u) == 0) {
            for (uint32_t m0 = 0; m0 < M; m0 += 16) {
                const uint4 w = *reinterpret_cast<const uint4*>(c + m0);
                const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
                for (uint32_t b = 0; b < 16; b++) {
                    const uint32_t code = (ws[b >> 2] >> ((b & 3) * 8)) & 0xFFu;
                    sum = sum + tab[(m0 + b) * Kt + code];
                }
            }
        } else {
            for (uint32_t m = 0; m < M; m++) sum = sum + tab[m * Kt + c[m]];
        }
        out[r] = f2u(-__builtin_sqrtf(sum));
    }
}

// BinaryThreshold::compute + BinaryVector::from_dense for row blockIdx.x (stride ld) -> words[row][W]
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t b = f2u(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// the element of rank `r` (0-based, ascending) of the row: radix select over the order-preserving keys, 8 bits per pass,
// histograms in LDS (-0.0 orders before +0.0 here while the reference's sort keeps them in input order; `v > t` is the
// same for either, so the bits are too)
__device__ float row_rank_value(const float* __restrict__ v, uint32_t dim, uint32_t r, uint32_t* hist, uint32_t* sh) {
    uint32_t prefix = 0, pmask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < dim; j += blockDim.x) {
            const uint32_t k = order_key(v[j]);
            if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 0xFFu], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t b = 0, below = 0;
            while (below + hist[b] <= r) below += hist[b++];
            sh[0] = b;
            sh[1] = r - below;
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        pmask |= 0xFFu << shift;
        r = sh[1];
        __syncthreads();
    }
    return key_value(prefix);
}

__global__ __launch_bounds__(256) void bq_quantize_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim, int method,
                                                          uint32_t W, uint64_t* __restrict__ words) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[2];
    __shared__ float s_thr;
    const float* v = rows + (uint64_t)blockIdx.x * ld;
    if (method == 1) {  // Mean: `vector.iter().sum::<f32>() / vector.len() as f32`
        if (threadIdx.x == 0) {
            float s = -0.0f;
            for (uint32_t j = 0; j < dim; j++) s = s + v[j];
            s_thr = s / (float)dim;
        }
    } else if (method == 2) {  // Median: sorted[mid] (odd) or sorted[mid - 1].midpoint(sorted[mid]) (even)
        const uint32_t mid = dim / 2;
        const float hi = row_rank_value(v, dim, mid, hist, sh);
        if (dim % 2 == 0) {
            const float lo = row_rank_value(v, dim, mid - 1, hist, sh);
            if (threadIdx.x == 0) s_thr = (float)(((double)lo + (double)hi) / 2.0);  // f32::midpoint on x86-64
        } else if (threadIdx.x == 0) {
            s_thr = hi;
        }
    } else if (threadIdx.x == 0) {
        s_thr = 0.0f;  // Sign
    }
    __syncthreads();
    const float t = s_thr;
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) {
        uint64_t word = 0;
        const uint32_t j0 = w * 64, j1 = min(dim, j0 + 64);
        for (uint32_t j = j0; j < j1; j++)
            if (v[j] > t) word |= 1ull << (j - j0);
        words[(uint64_t)blockIdx.x * W + w] = word;
    }
}

// BinaryVector::normalized_distance for the rows of one probed list / chunk / query (grid as pq_scan_kernel): the query's
// words are wave-uniform, each row XOR + popcount over its W words, `hamming as f32 / dim as f32`
__global__ __launch_bounds__(256) void bq_scan_kernel(const uint64_t* __restrict__ qwords, const uint64_t* __restrict__ codes, uint32_t W,
                                                      uint32_t dim, const CodecSeg* __restrict__ segs, uint32_t np,
                                                      const uint64_t* __restrict__ score_base, uint32_t* __restrict__ scores) {
    const uint32_t i = blockIdx.x, q = blockIdx.z;
    const CodecSeg sg = segs[(size_t)q * np + i];
    const uint32_t r0 = blockIdx.y * kCodecRowsPerBlock;
    if (r0 >= sg.count) return;
    const uint64_t* qw = qwords + (size_t)q * W;
    uint32_t* out = scores + score_base[q] + sg.cand;
    const uint32_t r1 = min(sg.count, r0 + kCodecRowsPerBlock);
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
        const uint64_t* c = codes + (uint64_t)(sg.start + r) * W;
        uint32_t h = 0;
        for (uint32_t w = 0; w < W; w++) h += (uint32_t)__popcll(qw[w] ^ c[w]);
        out[r] = f2u(-((float)h / (float)dim));
    }
}

}  // namespace

hipError_t launch_pq_residual(const float* rows, uint32_t ld_r, const float* cents, uint32_t ld_c, const uint32_t* assign, uint64_t n,
                              uint32_t dim, uint32_t subdim, float* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n * dim + 255) / 256, 8192);
    hipLaunchKernelGGL(pq_residual_kernel, dim3(blocks), dim3(256), 0, s, rows, ld_r, cents, ld_c, assign, n, dim, subdim, out);
    return hipGetLastError();
}

hipError_t launch_pq_encode(const float* res, uint64_t n, uint32_t M, uint32_t subdim, const float* cb, uint32_t K, uint8_t* codes,
                            hipStream_t s) {
    if (n == 0 || M == 0) return hipSuccess;
    const size_t lds = (size_t)K * subdim * 4;
    const dim3 grid((uint32_t)std::min<uint64_t>((n + 255) / 256, 1024), M);
    if (lds <= kLdsBudget) hipLaunchKernelGGL(pq_encode_kernel<true>, grid, dim3(256), lds, s, res, n, M, subdim, cb, K, codes);
    else hipLaunchKernelGGL(pq_encode_kernel<false>, grid, dim3(256), 0, s, res, n, M, subdim, cb, K, codes);
    return hipGetLastError();
}

size_t codec_seg_bytes() { return sizeof(CodecSeg); }

hipError_t launch_pq_search(const float* queries, uint32_t dim, const float* cents, uint32_t ld_c, const void* segs, uint32_t np,
                            uint32_t nq, uint32_t max_count, const float* cb, uint32_t K, uint32_t M, const uint8_t* codes,
                            float* tables, const uint64_t* score_base, uint32_t* scores, hipStream_t s) {
    if (nq == 0 || np == 0 || max_count == 0) return hipSuccess;
    const uint32_t Kt = std::min<uint32_t>(K, 256), subdim = dim / M;
    const CodecSeg* sg = static_cast<const CodecSeg*>(segs);
    if (Kt)
        hipLaunchKernelGGL(pq_table_kernel, dim3(np, nq), dim3(256), (size_t)dim * 4, s, queries, dim, cents, ld_c, sg, np, cb, K, Kt, M,
                           subdim, tables);
    const dim3 grid(np, (max_count + kCodecRowsPerBlock - 1) / kCodecRowsPerBlock, nq);
    const size_t lds = (size_t)M * Kt * 4;
    if (lds <= kLdsBudget) hipLaunchKernelGGL(pq_scan_kernel<true>, grid, dim3(256), lds, s, tables, codes, M, Kt, sg, np, score_base, scores);
    else hipLaunchKernelGGL(pq_scan_kernel<false>, grid, dim3(256), 0, s, tables, codes, M, Kt, sg, np, score_base, scores);
    return hipGetLastError();
}

hipError_t launch_bq_quantize(const float* rows, uint32_t ld, uint64_t n, uint32_t dim, int method, uint64_t* words, hipStream_t s) {
    const uint32_t W = (dim + 63) / 64;
    for (uint64_t r0 = 0; r0 < n; r0 += 65535) {  // (a workgroup per row)
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(65535, n - r0);
        hipLaunchKernelGGL(bq_quantize_kernel, dim3(cnt), dim3(256), 0, s, rows + r0 * ld, ld, dim, method, W, words + r0 * W);
    }
    return hipGetLastError();
}

hipError_t launch_bq_search(const uint64_t* qwords, uint32_t dim, const void* segs, uint32_t np, uint32_t nq, uint32_t max_count,
                            const uint64_t* codes, const uint64_t* score_base, uint32_t* scores, hipStream_t s) {
    if (nq == 0 || np == 0 || max_count == 0) return hipSuccess;
    const uint32_t W = (dim + 63) / 64;
    const dim3 grid(np, (max_count + kCodecRowsPerBlock - 1) / kCodecRowsPerBlock, nq);
    hipLaunchKernelGGL(bq_scan_kernel, grid, dim3(256), 0, s, qwords, codes, W, dim, static_cast<const CodecSeg*>(segs), np, score_base,
                       scores);
    return hipGetLastError();
}

}  // namespace nmn
