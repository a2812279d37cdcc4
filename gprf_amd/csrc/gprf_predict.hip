// gprf_predict.hip — GPRF prediction (GPRF.train_predictor / predict, gprf.py:593-672) on the device.
//
// A predictor holds, per block b of the training partition, a snapshot of the unary unit's W_b = U_b^-T (K_b^-1 = W_b^T W_b),
// alpha_b = K_b^-1 Y_b and the unit's point records (k_pred_gather).  A prediction is a set of GROUPS (test rows, at most
// PRED_MAX_T) with their SOURCE blocks; every (group, source) pair is a TASK.  Five launches, whatever the number of groups:
//   k_pred_stage copies the call's tables (staged in pinned host memory) into device memory
//   k_pred_kstar per (task, 16-column strip):  K*^T[:, strip] = k(X_i, X*[strip]), every value generated once
//   k_pred_v     per (task, 16-column strip, 16-row block r):  V_r = sum_{c <= r} W[r, c] K*[strip, c]^T   (V = W K*^T;
//                W is lower triangular: the blocks c > r are zero and skipped); one more item per strip: mean = K* alpha
//   k_pred_cov   per (task, 16 x 16 tile I >= J):   cov = Kss (+ nv I when test_noise_var > 0) - V_I^T V_J, lower tiles
//   k_pred_fuse  per group (one workgroup):  P = inv(prior) + sum_i (inv(cov_i) - inv(Kss)),  b = sum_i inv(cov_i) mean_i,
//                cov = inv(P), mean = cov b;  every inverse through a Cholesky factor (chol_inv below); the results are
//                stored straight into the caller's pinned host buffers
// The GEMM-shaped stages use the file-wide MFMA form of gprf_dev.h (D += SA^T SB, v_mfma_f64_16x16x4_f64).
#include <algorithm>

#include "gprf_dev.h"

namespace gprf {

namespace {

// a point record (the gathered form KernFn reads): XPAD doubles (euclidean) or the GEO_STRIDE-double half-angle record (lld)
template <int DIST>
__device__ __forceinline__ void load_rec(const double *__restrict__ src, double (&r)[GEO_STRIDE]) {
#pragma unroll
    for (int e = 0; e < GEO_STRIDE; ++e) r[e] = e < PtRec<DIST>::STRIDE ? src[e] : 0.0;
}

// ---- predictor build: the unary units' W, alpha and point records into the predictor's own pools ----
__global__ __launch_bounds__(256) void k_pred_gather(const PredGather *__restrict__ gl, const double *__restrict__ W,
                                                     const double *__restrict__ At, const double *__restrict__ Xu, int rs,
                                                     int dy, double *__restrict__ pW, double *__restrict__ pA,
                                                     double *__restrict__ pX) {
    const PredGather g = gl[blockIdx.x];
    const int m = g.m, mp = (m + 15) & ~15;
    const int64_t tot = (int64_t)mp * mp;
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.y * 256) {
        int i = (int)(e / mp), j = (int)(e % mp);
        pW[g.dst_mat + e] = (i < m && j <= i) ? W[g.src_mat + e] : 0.0;      // (only the lower triangle of W is defined)
    }
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < (int64_t)mp * YPAD; e += (int64_t)gridDim.y * 256) {
        int i = (int)(e / YPAD), d = (int)(e % YPAD);
        pA[(size_t)(g.dst_row + i) * YPAD + d] = (i < m && d < dy) ? At[(size_t)g.src_row * YPAD + (size_t)d * mp + i] : 0.0;
    }
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < (int64_t)mp * rs; e += (int64_t)gridDim.y * 256) {
        int i = (int)(e / rs), k = (int)(e % rs);
        // padding rows repeat row 0: a finite, valid record (their W columns / alpha rows are zero)
        pX[(size_t)(g.dst_row + i) * rs + k] = Xu[(size_t)(g.src_row + (i < m ? i : 0)) * rs + k];
    }
}

// ---- the call's tables: pinned host memory -> device memory (n16 16-byte words) ----
__global__ __launch_bounds__(256) void k_pred_stage(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n16; e += (size_t)gridDim.x * 256) dst[e] = src[e];
}

// ---- cross stage, part 0: K*^T (mp x tp per task, the layout of V), one value per (training point, test point) ----
template <int DIST, int KERN>
__global__ __launch_bounds__(256) void k_pred_kstar(PredArgs a) {
    const int4 it = a.items_k[blockIdx.x];
    const PredTask tk = a.tasks[it.x];
    const int s = it.y;
    constexpr int RS = PtRec<DIST>::STRIDE;
    const int j = threadIdx.x & 15;
    double xs[GEO_STRIDE];
    load_rec<DIST>(a.xs + (size_t)(tk.xs_row + 16 * s + j) * RS, xs);
    const double *__restrict__ xt = a.pX + (size_t)tk.b_row * RS;
    double *__restrict__ Kt = a.Kt + tk.v_off;
    for (int kk = threadIdx.x >> 4; kk < tk.mp; kk += 16)
        Kt[(size_t)kk * tk.tp + 16 * s + j] = KernFn<DIST, KERN>::value(a.kp, xt + (size_t)kk * RS, xs);
}

// ---- cross stage, part 1: V = W K*^T and mean = K* alpha ----
template <int DIST, int KERN>
__global__ __launch_bounds__(64) void k_pred_v(PredArgs a) {
    const int4 it = a.items_v[blockIdx.x];
    const PredTask tk = a.tasks[it.x];
    const int s = it.y, r = it.z;
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const double *__restrict__ Kt = a.Kt + tk.v_off + 16 * s + lr;      // K*^T[k][16s + lr] at Kt[k * tp]
    const int nrb = tk.mp / 16;
    if (r < nrb) {
        // D[i][j] = sum_k W[16r + i][k] K*[16s + j][k]:  a = W[16r + lr][16c + 4q + lg],  b = K*^T[16c + 4q + lg][16s + lr]
        const double *__restrict__ wrow = a.pW + tk.b_mat + (size_t)(16 * r + lr) * tk.mp;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c <= r; ++c) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kk = 16 * c + 4 * q + lg;
                acc = mfma(wrow[kk], Kt[(size_t)kk * tk.tp], acc);
            }
        }
        double *__restrict__ V = a.V + tk.v_off;
#pragma unroll
        for (int q = 0; q < 4; ++q) V[(size_t)(16 * r + lg + 4 * q) * tk.tp + 16 * s + lr] = acc[q];
    } else {
        // D[i][d] = sum_k K*[16s + i][k] alpha[k][d]:  a = K*^T[16c + 4q + lg][16s + lr],  b = alpha[16c + 4q + lg][16 db + lr]
        const double *__restrict__ al = a.pA + (size_t)tk.b_row * YPAD;
        const int ndb = (a.dy + 15) / 16;
        d4 acc[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) acc[db] = d4{0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < nrb; ++c) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kk = 16 * c + 4 * q + lg;
                const double kv = Kt[(size_t)kk * tk.tp];
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    if (db < ndb) acc[db] = mfma(kv, al[(size_t)kk * YPAD + 16 * db + lr], acc[db]);
            }
        }
        double *__restrict__ Mn = a.Mn + tk.mean_off;
#pragma unroll
        for (int db = 0; db < 4; ++db)
            if (db < ndb)
#pragma unroll
                for (int q = 0; q < 4; ++q) Mn[(size_t)(16 * s + lg + 4 * q) * YPAD + 16 * db + lr] = acc[db][q];
    }
}

// ---- cross stage, part 2: cov_i = Kss (+ nv I) - V^T V, the lower tiles (all the Cholesky reads) ----
template <int DIST, int KERN>
__global__ __launch_bounds__(64) void k_pred_cov(PredArgs a) {
    const int4 it = a.items_c[blockIdx.x];
    const PredTask tk = a.tasks[it.x];
    const int I = it.y, J = it.z;
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const double *__restrict__ V = a.V + tk.v_off;
    // D[i][j] = sum_k V[k][16I + i] V[k][16J + j]  (k = the training row)
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < tk.mp / 16; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t row = (size_t)(16 * r + 4 * q + lg) * tk.tp;
            acc = mfma(V[row + 16 * I + lr], V[row + 16 * J + lr], acc);
        }
    }
    constexpr int RS = PtRec<DIST>::STRIDE;
    double xj[GEO_STRIDE];
    const int j = 16 * J + lr;
    load_rec<DIST>(a.xs + (size_t)(tk.xs_row + j) * RS, xj);
    double *__restrict__ C = a.C + tk.c_off;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 16 * I + lg + 4 * q;
        if (i >= tk.t || j >= tk.t || j > i) continue;
        double xi[GEO_STRIDE];
        load_rec<DIST>(a.xs + (size_t)(tk.xs_row + i) * RS, xi);
        double kss = KernFn<DIST, KERN>::value(a.kp, xi, xj);
        if (i == j && a.test_nv > 0.0) kss += a.kp.nv;      // gprf.py:652-653 (the model's noise, whatever test_noise_var is)
        C[(size_t)i * tk.tp + j] = kss - acc[q];
    }
}

// ---- fuse stage helpers: one workgroup of PRED_NT threads; matrices t x t with leading dimension ld in global memory ----
constexpr int PRED_NT = 256;

__device__ __forceinline__ void wg_sync() { __syncthreads(); }

// A <- inv(A) for symmetric positive definite A, of which the lower triangle is read; the full square is written.
// A = L L^T (right-looking, in place), B = L^-1 (row by row), inv(A) = B^T B.  *bad = 1 if a pivot is not positive.
__device__ void chol_inv(double *__restrict__ A, double *__restrict__ B, int t, int ld, double *s_v, int *s_bad) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    constexpr int NW = PRED_NT / 64;
    for (int k = 0; k < t; ++k) {
        const double p = A[(size_t)k * ld + k];
        if (!(p > 0.0) && tid == 0) *s_bad = 1;
        const double d = sqrt(p);
        for (int i = k + tid; i < t; i += PRED_NT) {
            double v = i == k ? d : A[(size_t)i * ld + k] / d;
            s_v[i] = v;
        }
        wg_sync();
        for (int i = k + tid; i < t; i += PRED_NT) A[(size_t)i * ld + k] = s_v[i];
        for (int i = k + 1 + w; i < t; i += NW) {
            const double li = s_v[i];
            for (int j = k + 1 + lane; j <= i; j += 64) A[(size_t)i * ld + j] -= li * s_v[j];
        }
        wg_sync();
    }
    // B = L^-1:  B[i][i] = 1 / L[i][i],  B[i][j] = -(sum_{k=j}^{i-1} L[i][k] B[k][j]) / L[i][i]   (j < i)
    for (int i = 0; i < t; ++i) {
        for (int k = tid; k <= i; k += PRED_NT) s_v[k] = A[(size_t)i * ld + k];
        wg_sync();
        const double rd = 1.0 / s_v[i];
        for (int j = tid; j <= i; j += PRED_NT) {
            double v;
            if (j == i) {
                v = rd;
            } else {
                double sum = 0.0;
#pragma unroll 4
                for (int k = j; k < i; ++k) sum += s_v[k] * B[(size_t)k * ld + j];
                v = -sum * rd;
            }
            B[(size_t)i * ld + j] = v;
        }
        wg_sync();
    }
    // inv(A)[i][j] = sum_{k >= i} B[k][i] B[k][j]   (j <= i), mirrored
    for (int i = w; i < t; i += NW) {
        for (int j = lane; j <= i; j += 64) {
            double sum = 0.0;
#pragma unroll 4
            for (int k = i; k < t; ++k) sum += B[(size_t)k * ld + i] * B[(size_t)k * ld + j];
            A[(size_t)i * ld + j] = sum;
            A[(size_t)j * ld + i] = sum;
        }
    }
    wg_sync();
}

template <int DIST, int KERN>
__device__ void fill_kernel(double *__restrict__ A, const double *__restrict__ xs, int t, int ld, const KParams &kp,
                            double diag_add) {
    constexpr int RS = PtRec<DIST>::STRIDE;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = w; i < t; i += PRED_NT / 64) {
        double xi[GEO_STRIDE];
        load_rec<DIST>(xs + (size_t)i * RS, xi);
        for (int j = lane; j <= i; j += 64) {
            double xj[GEO_STRIDE];
            load_rec<DIST>(xs + (size_t)j * RS, xj);
            double v = KernFn<DIST, KERN>::value(kp, xi, xj);
            if (i == j) v += diag_add;
            A[(size_t)i * ld + j] = v;
        }
    }
    wg_sync();
}

template <int DIST, int KERN>
__global__ __launch_bounds__(PRED_NT) void k_pred_fuse(PredArgs a) {
    __shared__ double s_v[PRED_MAX_T];
    __shared__ int s_bad;
    const PredGroup g = a.groups[blockIdx.x];
    const int t = g.t, ld = g.tp, tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    wg_sync();
    double *__restrict__ P = a.ws + g.ws_off;
    double *__restrict__ A = P + (size_t)ld * ld;
    double *__restrict__ B = A + (size_t)ld * ld;
    double *__restrict__ bv = B + (size_t)ld * ld;      // t x YPAD
    const double *__restrict__ xs = a.xs + (size_t)g.xs_row * PtRec<DIST>::STRIDE;
    const int dy = a.dy;
    // P = inv(k_test(X*, X*) + test_noise_var I)                                             (gprf.py:623-625)
    fill_kernel<DIST, KERN>(A, xs, t, ld, a.kp_prior, a.test_nv);
    chol_inv(A, B, t, ld, s_v, &s_bad);
    for (int e = tid; e < t * t; e += PRED_NT) P[(size_t)(e / t) * ld + e % t] = A[(size_t)(e / t) * ld + e % t];
    for (int e = tid; e < t * YPAD; e += PRED_NT) bv[e] = 0.0;
    wg_sync();      // (P is read across waves below — by the last chol_inv when the group has no source)
    // every source's  - inv(Kss)  at once: Kss (+ nv I when test_noise_var > 0) is the same for all of them  (gprf.py:650-653,658)
    if (g.n_task > 0) {
        fill_kernel<DIST, KERN>(A, xs, t, ld, a.kp, a.test_nv > 0.0 ? a.kp.nv : 0.0);
        chol_inv(A, B, t, ld, s_v, &s_bad);
        const double ns = (double)g.n_task;
        for (int e = tid; e < t * t; e += PRED_NT) P[(size_t)(e / t) * ld + e % t] -= ns * A[(size_t)(e / t) * ld + e % t];
        wg_sync();
    }
    for (int k = 0; k < g.n_task; ++k) {
        const PredTask tk = a.tasks[g.task0 + k];
        double *__restrict__ C = a.C + tk.c_off;
        const double *__restrict__ Mn = a.Mn + tk.mean_off;
        chol_inv(C, B, t, ld, s_v, &s_bad);                                                // prec = inv(cov_i)  (gprf.py:657)
        for (int e = tid; e < t * t; e += PRED_NT) P[(size_t)(e / t) * ld + e % t] += C[(size_t)(e / t) * ld + e % t];
        for (int e = tid; e < t * dy; e += PRED_NT) {                                     // b += prec mean_i  (gprf.py:660-661)
            const int i = e / dy, d = e % dy;
            double sum = 0.0;
            for (int j = 0; j < t; ++j) sum += C[(size_t)i * ld + j] * Mn[(size_t)j * YPAD + d];
            bv[(size_t)i * YPAD + d] += sum;
        }
        wg_sync();
    }
    // cov = inv(P), mean = cov b                                                            (gprf.py:664-665)
    chol_inv(P, B, t, ld, s_v, &s_bad);
    double *__restrict__ cov = a.cov_out + g.cov_off;
    double *__restrict__ mean = a.mean_out + g.mean_off;
    for (int e = tid; e < t * t; e += PRED_NT) cov[e] = P[(size_t)(e / t) * ld + e % t];
    for (int e = tid; e < t * dy; e += PRED_NT) {
        const int i = e / dy, d = e % dy;
        double sum = 0.0;
        for (int j = 0; j < t; ++j) sum += P[(size_t)i * ld + j] * bv[(size_t)j * YPAD + d];
        mean[e] = sum;
    }
    if (tid == 0) a.status[blockIdx.x] = s_bad;
}

template <int DIST, int KERN>
void launch_predict_t(const PredArgs &a, int n_items_k, int n_items_v, int n_items_c, int n_groups, hipStream_t s) {
    if (n_items_k > 0) hipLaunchKernelGGL((k_pred_kstar<DIST, KERN>), dim3(n_items_k), dim3(256), 0, s, a);
    if (n_items_v > 0) hipLaunchKernelGGL((k_pred_v<DIST, KERN>), dim3(n_items_v), dim3(64), 0, s, a);
    if (n_items_c > 0) hipLaunchKernelGGL((k_pred_cov<DIST, KERN>), dim3(n_items_c), dim3(64), 0, s, a);
    if (n_groups > 0) hipLaunchKernelGGL((k_pred_fuse<DIST, KERN>), dim3(n_groups), dim3(PRED_NT), 0, s, a);
}

}  // namespace

void launch_pred_gather(const PredGather *gl, int n, const double *W, const double *At, const double *Xu, int rs, int dy,
                        double *pW, double *pA, double *pX, int max_m, hipStream_t s) {
    if (n <= 0) return;
    const int ysplit = std::max(1, std::min(64, (max_m * max_m) / (256 * 64)));
    hipLaunchKernelGGL(k_pred_gather, dim3(n, ysplit), dim3(256), 0, s, gl, W, At, Xu, rs, dy, pW, pA, pX);
}

void launch_predict(int dist_id, const PredArgs &a, const void *tab_src, size_t tab_bytes, int n_items_k, int n_items_v,
                    int n_items_c, int n_groups, hipStream_t s) {
    const size_t n16 = tab_bytes / 16;
    if (n16 > 0)
        hipLaunchKernelGGL(k_pred_stage, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 1024)), dim3(256), 0, s,
                           (const uint4 *)tab_src, (uint4 *)a.tasks, n16);
    if (dist_id == 1) launch_predict_t<1, 1>(a, n_items_k, n_items_v, n_items_c, n_groups, s);
    else launch_predict_t<0, 0>(a, n_items_k, n_items_v, n_items_c, n_groups, s);
}

}  // namespace gprf
