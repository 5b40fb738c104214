// Log-weights method, M <= 1024: the dual Newton minimizer with the nuisance scales profiled out (gfx950).  Rows
// belong to groups (group[i] in -1, 0 .. p - 1; -1: the scale stays 1), a group has ONE least-squares scale
//   s_k = sum_{i in k} ybar_i (YT_i - off_i) / sum_{i in k} ybar_i^2          (ybar = Y w, the RAW averages)
// and sigma_i = s_group(i) is the affine model's row_scale for the rest of the evaluation, of the Gram finish and of the step.
//   k_rows_combine_profile   k_rows_combine<true>'s job for K = 1 in one block, the scales formed between the segments'
//                            shares and the rows' finish
//   k_lproj_vhat .. _apply   behind k_lgram_finish: C_A, -b_A -> Pi C_A Pi, -Pi b_A, Pi = I - sum_k vhat_k vhat_k^T, vhat_k =
//                            ybar restricted to group k, normalised
// Every sum over a group's rows has ONE order, fixed by the rows and the groups alone: lane l of the group's wave takes rows
// l, l + 64, ... in turn, the lanes meet in wave_sum's pair order.  No atomics; the same bits call after call.
#include "device_utils.hpp"
#include "kernels.hpp"

namespace bioen {

constexpr int kProfRows = 1024;      // what dense_guard admits (mp <= 1024)

// sum over the rows of group k of a(row) b(row), by the calling wave (all 64 lanes); the result in every lane
template <class A, class B>
__device__ __forceinline__ double group_dot(const int* __restrict__ grp, int k, int rows, A a, B b) {
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int row = lane; row < rows; row += 64)
        if (grp[row] == k) s = fma(a(row), b(row), s);
    return wave_sum(s);
}

// One block.  The softmax normalisation over the segments and the segments' shares of the raw ybar exactly as
// k_rows_combine<true> forms them (the factors e^{m_v - M} / S, the shares added by fma in segment order); then the p
// pairs (numerator, denominator), s_k -> scales, sigma -> row_scale; then that kernel's finish of the rows and its scalars.
// group: mp entries, the padding rows -1.
__global__ __launch_bounds__(kBlock) void k_rows_combine_profile(Xch xi, int mp, const double* __restrict__ YT,
                                                                 const double* __restrict__ row_offset,
                                                                 const double* __restrict__ center,
                                                                 const int* __restrict__ group, int ngroups,
                                                                 double* __restrict__ row_scale, double* __restrict__ scales,
                                                                 double* __restrict__ ybar_c, double* __restrict__ r_c,
                                                                 double* __restrict__ sc, double theta) {
    __shared__ double sh[kWaves];
    __shared__ double fac[kShRed];
    __shared__ double raw[kProfRows];
    __shared__ int grp[kProfRows];
    __shared__ double sk[64];
    const size_t tail_at = (size_t)mp;
    double gmax = -DBL_MAX, S = 0.0, PP = 0.0;
    for (int r = 0; r < xi.world; ++r) gmax = fmax(gmax, xi.base[(size_t)r * xi.payload + tail_at + 2]);
    for (int r = 0; r < xi.world; ++r) {
        const double* tail = xi.base + (size_t)r * xi.payload + tail_at;
        const double fr = exp(tail[2] - gmax);
        S = fma(fr, tail[0], S);
        PP = fma(fr, tail[1], PP);
    }
    const double invS = 1.0 / S;
    for (int r = threadIdx.x; r < xi.world; r += kBlock)
        fac[r] = exp(xi.base[(size_t)r * xi.payload + tail_at + 2] - gmax) * invS;
    __syncthreads();
    if (threadIdx.x == 0) {
        sc[S_LOGS] = gmax + log(S);
        sc[S_P] = PP * invS;
    }
    if ((int)threadIdx.x < xi.vr) sc[S_INV + threadIdx.x] = fac[xi.rank + threadIdx.x];
    // the raw averages
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        double s = 0.0;
        for (int r = 0; r < xi.world; ++r) s = fma(fac[r], xi.base[(size_t)r * xi.payload + row], s);
        raw[row] = s + (center ? center[row] : 0.0);
        grp[row] = group[row];
    }
    __syncthreads();
    // the scales: group k is wave k mod kWaves's
    const int wave = threadIdx.x >> 6;
    for (int k = wave; k < ngroups; k += kWaves) {
        const double num = group_dot(grp, k, mp, [&](int row) { return raw[row]; },
                                     [&](int row) { return YT[row] - row_offset[row]; });
        const double den = group_dot(grp, k, mp, [&](int row) { return raw[row]; }, [&](int row) { return raw[row]; });
        if ((threadIdx.x & 63) == 0) {
            const double s = num / den;      // den = 0 or not finite: s, and with it f, is not finite -- the loop's rules apply
            sk[k] = s;
            scales[k] = s;
        }
    }
    __syncthreads();
    // the rows' finish: k_rows_combine's arithmetic with sc = sigma
    double chi = 0.0, cc = 0.0, b0 = 0.0, uy = 0.0;
    for (int row = threadIdx.x; row < mp; row += kBlock) {
        const int g = grp[row];
        const double sg = g >= 0 ? sk[g] : 1.0;
        const double cen = center ? center[row] : 0.0;
        const double rw = raw[row];
        const double eff = fma(sg, rw, row_offset[row]);
        const double res = eff - YT[row];
        row_scale[row] = sg;
        ybar_c[row] = rw;
        r_c[row] = res * sg;
        chi = fma(res, res, chi);
        cc = fma(eff, res, cc);
        b0 = fma(cen, res * sg, b0);
        uy = fma(rw, res * sg, uy);
    }
    chi = block_sum(chi, sh);
    cc = block_sum(cc, sh);
    b0 = block_sum(b0, sh);
    uy = block_sum(uy, sh);
    if (threadIdx.x == 0) {
        sc[S_CHI] = chi;
        sc[S_C] = cc;
        sc[S_B0] = b0;
        sc[S_UY] = uy;
        sc[S_KL] = sc[S_P] - sc[S_LOGS] + sc[S_LOGS0];
        sc[S_F] = theta * sc[S_KL] + 0.5 * chi;
    }
}

// One block: vhat_i = ybar_i / sqrt(sum_{i in group} ybar_i^2), 0 for a row in no group
__global__ __launch_bounds__(kBlock) void k_lproj_vhat(int m, const int* __restrict__ group, int ngroups,
                                                       const double* __restrict__ ybar, double* __restrict__ vhat) {
    __shared__ double inv[64];
    const int wave = threadIdx.x >> 6;
    for (int k = wave; k < ngroups; k += kWaves) {
        const double den = group_dot(group, k, m, [&](int row) { return ybar[row]; }, [&](int row) { return ybar[row]; });
        if ((threadIdx.x & 63) == 0) inv[k] = 1.0 / sqrt(den);
    }
    __syncthreads();
    for (int row = threadIdx.x; row < m; row += kBlock) {
        const int g = group[row];
        vhat[row] = g >= 0 ? ybar[row] * inv[g] : 0.0;
    }
}

// T[k][j] = sum_{i in k} vhat_i C_ij (j < m), T[k][m] = sum_{i in k} vhat_i negb_i; ldt = m + 1.  blockIdx.y = k, a block =
// 64 columns x 4 parts: part t adds its rows t, t + 4, ... in turn, the parts meet as (s0 + s1) + (s2 + s3)
__global__ __launch_bounds__(kBlock) void k_lproj_T(int m, const int* __restrict__ group, const double* __restrict__ vhat,
                                                    const double* __restrict__ cov, const double* __restrict__ negb,
                                                    double* __restrict__ T) {
    __shared__ double part[kWaves][64];
    const int k = blockIdx.y, lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (j <= m)
        for (int i = t; i < m; i += kWaves)
            if (group[i] == k) s = fma(vhat[i], j < m ? cov[(size_t)i * m + j] : negb[i], s);
    part[t][lane] = s;
    __syncthreads();
    if (t == 0 && j <= m) T[(size_t)k * (m + 1) + j] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// q[k][h] = sum_{j in h} T[k][j] vhat_j; blockIdx.x = k, group h is wave h mod kWaves's
__global__ __launch_bounds__(kBlock) void k_lproj_q(int m, const int* __restrict__ group, int ngroups,
                                                    const double* __restrict__ vhat, const double* __restrict__ T,
                                                    double* __restrict__ q) {
    const int k = blockIdx.x, wave = threadIdx.x >> 6;
    const double* Tk = T + (size_t)k * (m + 1);
    for (int h = wave; h < ngroups; h += kWaves) {
        const double s = group_dot(group, h, m, [&](int row) { return Tk[row]; }, [&](int row) { return vhat[row]; });
        if ((threadIdx.x & 63) == 0) q[k * 64 + h] = s;
    }
}

// In place on the lower triangle, mirrored (k_lgram_finish's grid): C_ij - vhat_i T[g(i)][j] - T[g(j)][i] vhat_j + vhat_i
// q[g(i)][g(j)] vhat_j -- an element reads C at itself alone --; the blocks of tile column 0 project -b
__global__ __launch_bounds__(256) void k_lproj_apply(int m, const int* __restrict__ group, const double* __restrict__ vhat,
                                                     const double* __restrict__ T, const double* __restrict__ q,
                                                     double* __restrict__ cov, double* __restrict__ negb) {
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= m || j > i) return;
    const int gi = group[i], gj = group[j];
    const double vi = vhat[i], vj = vhat[j];
    const int ldt = m + 1;
    double cv = cov[(size_t)i * m + j];
    if (gi >= 0) cv = fma(-vi, T[(size_t)gi * ldt + j], cv);
    if (gj >= 0) cv = fma(-T[(size_t)gj * ldt + i], vj, cv);
    if (gi >= 0 && gj >= 0) cv = fma(vi * q[gi * 64 + gj], vj, cv);
    cov[(size_t)i * m + j] = cv;
    cov[(size_t)j * m + i] = cv;
    if (j == 0 && gi >= 0) negb[i] = fma(-vi, T[(size_t)gi * ldt + m], negb[i]);
}

// ---- host side ------------------------------------------------------------------------------------
size_t logw_profile_doubles(const bioen_hip_ctx* c) {
    return 64 + (size_t)c->mp + 64 * 64 + (size_t)64 * (c->mp + 1) + (size_t)(c->mp + 1) / 2;
}

LogwProfileBuf logw_profile_layout(const bioen_hip_ctx* c, double* base) {
    LogwProfileBuf b;
    b.scales = base;
    b.vhat = b.scales + 64;
    b.q = b.vhat + c->mp;
    b.T = b.q + 64 * 64;
    b.group = reinterpret_cast<int*>(b.T + (size_t)64 * (c->mp + 1));
    return b;
}

void launch_rows_combine_profile(bioen_hip_ctx* c, const Round& r, const double* center) {
    const LogwProfileBuf b = logw_profile_layout(c, c->scratch[SCRATCH_LOGW_PROFILE].p);
    hipLaunchKernelGGL(k_rows_combine_profile, dim3(1), dim3(kBlock), 0, c->stream,
                       make_xch(c, X_YBAR, ybar_payload(c, 1, true)), c->mp, c->YT, c->row_offset, center, b.group,
                       c->profile_groups, c->row_scale, b.scales, c->ybar_c, c->r_c, r.scal[0], r.theta[0]);
}

void launch_logw_project(bioen_hip_ctx* c, const double* ybar, double* cov, double* negb) {
    const LogwProfileBuf b = logw_profile_layout(c, c->scratch[SCRATCH_LOGW_PROFILE].p);
    const int m = c->m, p = c->profile_groups;
    hipLaunchKernelGGL(k_lproj_vhat, dim3(1), dim3(kBlock), 0, c->stream, m, b.group, p, ybar, b.vhat);
    hipLaunchKernelGGL(k_lproj_T, dim3((m + 1 + 63) / 64, p), dim3(kBlock), 0, c->stream, m, b.group, b.vhat, cov,
                       negb, b.T);
    hipLaunchKernelGGL(k_lproj_q, dim3(p), dim3(kBlock), 0, c->stream, m, b.group, p, b.vhat, b.T, b.q);
    const int tb = (m + 15) / 16;
    hipLaunchKernelGGL(k_lproj_apply, dim3(tb, tb), dim3(256), 0, c->stream, m, b.group, b.vhat, b.T, b.q, cov, negb);
}

}  // namespace bioen
