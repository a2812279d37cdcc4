// gprf_kernelized.hip — the unit arithmetic of kernelized observations (gaussian_llgrad_kernel, gprf.py:674-736): the outputs
// are known only through their n x n Gram matrix YY, resident in HBM.  Behind the Cholesky and the substitution (W = U^-T,
// no right-hand side) every unit forms, with YYu = YY[rows][:, rows] gathered through upt:
//   G = W YYu                      (U pool)      tr(P YYu) = sum G o W  -> zzpart (the ll term the plain path takes from ||Z||^2)
//   S = G W^T                      (K pool)
//   H = S W - dy W = (S - dy I) W  (U pool, over G)
//   M = W^T H, lower tiles         (K pool, over S)  = P YYu P - dy P  with P = K^-1 = W^T W
// and k_mgrad's "M from memory" form reduces M against dk/dx, dk/dtheta exactly as it does the plain path's A A^T - dy P.
// fp64 throughout, one MFMA form (v_mfma_f64_16x16x4_f64): a wave owns one 16 x 16 output tile.
#include "gprf_dev.h"

namespace gprf {

namespace {

// a W entry of a real point pair on or below the diagonal; everything else (the never-written strictly-upper tiles, the upper
// half of a diagonal tile, the padding rows) reads as zero
__device__ __forceinline__ double w_at(const double *__restrict__ W, int mp, int m, int r, int c) {
    return (r < m && c <= r) ? W[(size_t)r * mp + c] : 0.0;
}

// MODE 0: G = W YYu        (all tiles, k tiles 0..P)
// MODE 1: S = G W^T        (all tiles, k tiles 0..Q)
// MODE 2: H = S W - dy W   (all tiles, k tiles Q..T-1)
// MODE 3: M = W^T H        (tiles P >= Q, k tiles P..T-1)
// Grid: n_ids x wpu workgroups, wpu = ceil(max_T^2 / 4); workgroup slot * wpu + r, wave w -> tile 4 r + w = P max_T + Q.
template <int MODE>
__global__ __launch_bounds__(256) void k_kz_gemm(UnitTab ut, Pools pl, const double *__restrict__ YY, int n, double dy, int wpu) {
    const int slot = (int)blockIdx.x / wpu;
    if (slot >= ut.n_ids) return;
    const int r = (int)blockIdx.x - slot * wpu;
    const UnitRef ur = unit_ref(ut.srec, slot);
    const int m = ur.m, mp = pad16(m), T = mp >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int t = 4 * r + wave;
    const int P = t / ut.max_T, Q = t - P * ut.max_T;
    if (P >= T || Q >= T) return;      // (wave-uniform; no barrier below)
    if (MODE == 3 && Q > P) return;
    const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
    const double *__restrict__ W = pl.W + ur.mat_off;
    const double *__restrict__ Gs = pl.U + ur.mat_off;      // G (MODE 1 reads it), H (MODE 3 reads it)
    const double *__restrict__ Ss = pl.K + ur.mat_off;      // S (MODE 2 reads it)
    const int32_t *__restrict__ upt = ut.upt + ur.row_off;
    double *__restrict__ out = (MODE == 0 || MODE == 2) ? pl.U + ur.mat_off : pl.K + ur.mat_off;
    const int i0 = 16 * P, j0 = 16 * Q;
    d4 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = (MODE == 2) ? -dy * w_at(W, mp, m, i0 + lg + 4 * q, j0 + lr) : 0.0;
    int k0t, k1t;      // k tiles [k0t, k1t)
    if (MODE == 0) { k0t = 0; k1t = P + 1; }
    else if (MODE == 1) { k0t = 0; k1t = Q + 1; }
    else if (MODE == 2) { k0t = Q; k1t = T; }
    else { k0t = P; k1t = T; }
    // MODE 0: the B column's point, fixed for the lane
    const int jq = j0 + lr;
    const size_t ycol = (MODE == 0 && jq < m) ? (size_t)upt[jq] : 0;
    for (int kt = k0t; kt < k1t; ++kt) {
        double a[4], b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * kt + 4 * s + lg;      // this lane's k of MFMA s
            const int i = i0 + lr;                   // A row (output row), B column j = j0 + lr
            if (MODE == 0) {
                a[s] = w_at(W, mp, m, i, k);
                b[s] = (k < m && jq < m) ? YY[(size_t)upt[k] * (size_t)n + ycol] : 0.0;
            } else if (MODE == 1) {
                a[s] = Gs[(size_t)i * mp + k];
                b[s] = w_at(W, mp, m, jq, k);
            } else if (MODE == 2) {
                a[s] = Ss[(size_t)i * mp + k];
                b[s] = w_at(W, mp, m, k, jq);
            } else {
                a[s] = w_at(W, mp, m, k, i);
                b[s] = Gs[(size_t)k * mp + jq];
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma(a[s], b[s], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(size_t)(i0 + lg + 4 * q) * mp + j0 + lr] = acc[q];
}

// tr(P YYu) = sum_{p, k <= p} G[p][k] W[p][k], one workgroup per unit, fixed order (bit-reproducible) -> zzpart[u] = (tr, 0, 0, 0)
__global__ __launch_bounds__(256) void k_kz_trace(UnitTab ut, Pools pl) {
    const int slot = blockIdx.x;
    if (slot >= ut.n_ids) return;
    const UnitRef ur = unit_ref(ut.srec, slot);
    const int m = ur.m, mp = pad16(m);
    const double *__restrict__ W = pl.W + ur.mat_off;
    const double *__restrict__ G = pl.U + ur.mat_off;
    __shared__ double red[256];
    double s = 0.0;
    const int64_t tot = (int64_t)m * m;
    for (int64_t e = threadIdx.x; e < tot; e += 256) {
        const int p = (int)(e / m), k = (int)(e - (int64_t)p * m);
        if (k <= p) s += G[(size_t)p * mp + k] * W[(size_t)p * mp + k];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 4) pl.zzpart[(size_t)ur.u * 4 + threadIdx.x] = threadIdx.x == 0 ? red[0] : 0.0;
}

}  // namespace

void launch_kz_products(const UnitTab &ut, const Pools &p, const double *YY, int n, double dy, bool want_M, hipStream_t s) {
    if (ut.n_ids == 0 || ut.max_T == 0) return;
    const int wpu = (ut.max_T * ut.max_T + 3) / 4;
    const dim3 grid((unsigned)((size_t)ut.n_ids * wpu)), blk(256);
    hipLaunchKernelGGL(k_kz_gemm<0>, grid, blk, 0, s, ut, p, YY, n, dy, wpu);
    hipLaunchKernelGGL(k_kz_trace, dim3(ut.n_ids), blk, 0, s, ut, p);
    if (!want_M) return;
    hipLaunchKernelGGL(k_kz_gemm<1>, grid, blk, 0, s, ut, p, YY, n, dy, wpu);
    hipLaunchKernelGGL(k_kz_gemm<2>, grid, blk, 0, s, ut, p, YY, n, dy, wpu);
    hipLaunchKernelGGL(k_kz_gemm<3>, grid, blk, 0, s, ut, p, YY, n, dy, wpu);
}

}  // namespace gprf
