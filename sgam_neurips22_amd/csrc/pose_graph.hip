// pose_graph.hip — multiway registration: the pose graph over pairwise registrations, optimised on the device by Levenberg-Marquardt
// with a line process on the uncertain edges (Choi, Zhou, Koltun, CVPR 2015; Open3D's GlobalOptimizationLevenbergMarquardt as
// documented, unpinned), and the dense fp64 SPD solve it needs.  Poses, optimiser state and history live on the device, as in
// point_icp.hip: an attempt is a fixed sequence of launches and reads nothing back.  The model and every rule are stated in
// include/sgam_hip.h; tests/posegraph_oracle.py restates them in numpy.  No atomics; every output is a function of the inputs.
// Built with -ffp-contract=off: every operator below is one IEEE operation, except inside the solve, whose fused operations are
// explicit (__builtin_fma, the MFMA).  DESIGN §4.4.11.
//
// State: 16 DEVICE doubles: [0] lambda, [1] nu, [2] F, [3] status (0 running, 1 converged, 2 degenerate), [4] accepted iterations,
// [5] attempts, [6] live (this attempt passed the gate), [7] accepted (this attempt's trial was taken), [8] fold: F', [9] fold:
// delta . (lambda delta + b), [10] max |b|, [11] mu, [12..15] 0.
//
// Solve: A + lambda I = L L^T, right-looking in 64-column panels on a padded copy W (np = 64 ceil(n / 64); the padding is the
// identity): the diagonal tile in LDS by one workgroup, the tiles below it by a triangular solve (one lane per row), the trailing
// tiles by v_mfma_f64_16x16x4_f64 (fragment layout: feature_metrics.hip), then blocked forward and back substitution.  Every
// kernel returns when the status word is not 0; a failed pivot sets it to 2.
#include "points_common.h"

#include <cmath>

namespace {

constexpr int PG_MAX_NODES = 1024, PG_MAX_EDGES = 65536, SPD_MAX_N = 6144;
constexpr int PG_ROW = 8;              // doubles of a history row
enum { S_LAMBDA = 0, S_NU, S_COST, S_STATUS, S_ITER, S_ATTEMPTS, S_LIVE, S_ACCEPTED, S_TRIAL_COST, S_DENOM, S_GMAX, S_MU };
constexpr double PG_TAU = 1e-5;
constexpr double PG_PIVOT_REL = 1e-12;        // point_icp.hip's ICP_PIVOT_REL
constexpr double PG_SMALL_THETA2 = 1e-16;     // point_icp.hip's ICP_SMALL_THETA2

// ---------------------------------------------------------------- rigid 3 x 4 arithmetic (rows 0..2 of a row-major 4 x 4)
__device__ __forceinline__ void inv_rigid(const double *__restrict__ P, double (&A)[12]) {
    A[0] = P[0]; A[1] = P[4]; A[2] = P[8];
    A[4] = P[1]; A[5] = P[5]; A[6] = P[9];
    A[8] = P[2]; A[9] = P[6]; A[10] = P[10];
    A[3] = -((P[0] * P[3] + P[4] * P[7]) + P[8] * P[11]);
    A[7] = -((P[1] * P[3] + P[5] * P[7]) + P[9] * P[11]);
    A[11] = -((P[2] * P[3] + P[6] * P[7]) + P[10] * P[11]);
}

template <typename X, typename Y>
__device__ __forceinline__ void mul_rigid(const X &x, const Y &y, double (&Z)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double t = (x[r * 4] * y[c] + x[r * 4 + 1] * y[4 + c]) + x[r * 4 + 2] * y[8 + c];
            if (c == 3) t = t + x[r * 4 + 3];
            Z[r * 4 + c] = t;
        }
    }
}

// sum_b M[b] * v[b] in ascending b, the first product the start of the sum
#define PG_DOT6(expr_m, expr_v)                                  \
    ([&]() {                                                     \
        double t_;                                               \
        { const int b = 0; t_ = (expr_m) * (expr_v); }           \
        _Pragma("unroll") for (int b = 1; b < 6; ++b) t_ = t_ + (expr_m) * (expr_v); \
        return t_;                                               \
    }())

// one lane per edge: r, J, q, l, the cost term, K = J^T W J and g = J^T W r
__global__ __launch_bounds__(64) void pg_linearize_kernel(const double *__restrict__ poses, const int32_t *__restrict__ src,
                                                          const int32_t *__restrict__ dst, const double *__restrict__ Tst,
                                                          const double *__restrict__ info, const uint8_t *__restrict__ uncertain, int E,
                                                          const double *__restrict__ state, double *__restrict__ r_out,
                                                          double *__restrict__ J_out, double *__restrict__ q_out, double *__restrict__ l_out,
                                                          double *__restrict__ cost_out, double *__restrict__ K_out, double *__restrict__ g_out) {
    if (state[S_STATUS] != 0.0) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double mu = state[S_MU];
    const double *Ps = poses + (int64_t)src[e] * 16, *Pt = poses + (int64_t)dst[e] * 16;
    double A[12], Ti[12], B[12], M[12];
    inv_rigid(Pt, A);
    inv_rigid(Tst + e * 16, Ti);
    mul_rigid(Ps, Ti, B);
    mul_rigid(A, B, M);
    double r[6] = {(M[9] - M[6]) * 0.5, (M[2] - M[8]) * 0.5, (M[4] - M[1]) * 0.5, M[3], M[7], M[11]};
    double J[6][6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        double Q[12];                                     // A G_k B for the rotation generator k: rows of A against e_k x (columns of B)
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
            for (int c = 0; c < 4; ++c) Q[rr * 4 + c] = A[rr * 4 + k2] * B[k1 * 4 + c] - A[rr * 4 + k1] * B[k2 * 4 + c];
        }
        J[0][k] = (Q[9] - Q[6]) * 0.5; J[1][k] = (Q[2] - Q[8]) * 0.5; J[2][k] = (Q[4] - Q[1]) * 0.5;
        J[3][k] = Q[3]; J[4][k] = Q[7]; J[5][k] = Q[11];
        J[0][3 + k] = 0.0; J[1][3 + k] = 0.0; J[2][3 + k] = 0.0;      // translation generator k: [0 | column k of A's rotation]
        J[3][3 + k] = A[k]; J[4][3 + k] = A[4 + k]; J[5][3 + k] = A[8 + k];
    }
    double L[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) L[a][b] = info[e * 36 + a * 6 + b];
    }
    double y[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) y[a] = PG_DOT6(L[a][b], r[b]);
    const double q = PG_DOT6(r[b], y[b]);
    double l = 1.0;
    if (uncertain[e]) {
        const double t = mu / (mu + q);
        l = t * t;
    }
    double cost = l * q;
    if (uncertain[e]) {
        const double d = sqrt(l) - 1.0;
        cost = cost + mu * (d * d);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) L[a][b] = l * L[a][b];            // W = l Lambda
    }
    double wr[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) wr[a] = PG_DOT6(L[a][b], r[b]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double wj[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) wj[a] = PG_DOT6(L[a][b], J[b][k]);
#pragma unroll
        for (int j = 0; j < 6; ++j) K_out[e * 36 + j * 6 + k] = PG_DOT6(J[b][j], wj[b]);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) g_out[e * 6 + j] = PG_DOT6(J[b][j], wr[b]);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        r_out[e * 6 + a] = r[a];
#pragma unroll
        for (int b = 0; b < 6; ++b) J_out[e * 36 + a * 6 + b] = J[a][b];
    }
    q_out[e] = q; l_out[e] = l; cost_out[e] = cost;
}

// ---------------------------------------------------------------- assembly
// gate of the kernels an attempt runs after its decision: the prologue (gated == 0) runs whenever the state is live
__device__ __forceinline__ bool pg_skip(const double *__restrict__ state, int gated) {
    return state[S_STATUS] != 0.0 || (gated && state[S_ACCEPTED] == 0.0);
}

__global__ __launch_bounds__(256) void pg_zero_kernel(double *__restrict__ H, int64_t count, const double *__restrict__ state, int gated) {
    if (pg_skip(state, gated)) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) H[i] = 0.0;
}

// one workgroup of 64 lanes per listed 6 x 6 block (row a <= column c): lane < 36 sums entry (lane / 6, lane % 6) over the block's
// edges in list order (ascending edge index); lanes 36..41 of a diagonal block sum the node's b
__global__ __launch_bounds__(64) void pg_gather_kernel(const double *__restrict__ K, const double *__restrict__ g, int N, int fixed,
                                                       const int32_t *__restrict__ block_row, const int32_t *__restrict__ block_col,
                                                       const int32_t *__restrict__ block_ptr, const int32_t *__restrict__ block_entry,
                                                       const double *__restrict__ state, int gated, double *__restrict__ H,
                                                       double *__restrict__ bvec) {
    if (pg_skip(state, gated)) return;
    const int blk = blockIdx.x, lane = threadIdx.x;
    const int a = block_row[blk], c = block_col[blk];
    const int lo = block_ptr[blk], hi = block_ptr[blk + 1];
    const int64_t n = (int64_t)N * 6;
    const bool pinned = a == fixed || c == fixed;
    if (lane < 36) {
        const int i = lane / 6, j = lane % 6;
        double h = 0.0;
        if (pinned) {
            h = (a == c && i == j) ? 1.0 : 0.0;
        } else if (a == c) {
            for (int p = lo; p < hi; ++p) h = h + K[(int64_t)(block_entry[p] >> 1) * 36 + i * 6 + j];
        } else {
            for (int p = lo; p < hi; ++p) {
                const int en = block_entry[p];
                const double *Ke = K + (int64_t)(en >> 1) * 36;
                h = h - ((en & 1) ? Ke[j * 6 + i] : Ke[i * 6 + j]);
            }
        }
        H[((int64_t)a * 6 + i) * n + (int64_t)c * 6 + j] = h;
        if (a != c) H[((int64_t)c * 6 + j) * n + (int64_t)a * 6 + i] = h;
    } else if (lane < 42 && a == c) {
        const int i = lane - 36;
        double t = 0.0;
        if (!pinned) {
            for (int p = lo; p < hi; ++p) {
                const int en = block_entry[p];
                const double ge = g[(int64_t)(en >> 1) * 6 + i];
                t = (en & 1) ? t + ge : t - ge;
            }
        }
        bvec[(int64_t)a * 6 + i] = t;
    }
}

// ---------------------------------------------------------------- the folds of an attempt
// the fixed-order fold of one workgroup: lane t takes the items t, t + 256, ... in ascending order, then the 256 lane sums are
// halved in LDS: s[t] = s[t] + s[t + h] for h = 128, 64, ..., 1
__device__ __forceinline__ double pg_tree_sum(double v, double *__restrict__ lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) lds[t] = lds[t] + lds[t + h];
        __syncthreads();
    }
    return lds[0];
}

__global__ __launch_bounds__(256) void pg_fold_kernel(const double *__restrict__ cost, int E, const double *__restrict__ delta,
                                                      const double *__restrict__ bvec, int n, double *__restrict__ state) {
    __shared__ double lds[256];
    if (state[S_STATUS] != 0.0) return;
    double f = 0.0, d = 0.0;
    for (int e = threadIdx.x; e < E; e += 256) f = f + cost[e];
    if (delta) {
        const double lambda = state[S_LAMBDA];
        for (int i = threadIdx.x; i < n; i += 256) d = d + delta[i] * (lambda * delta[i] + bvec[i]);
    }
    f = pg_tree_sum(f, lds);
    d = pg_tree_sum(d, lds);
    if (threadIdx.x == 0) { state[S_TRIAL_COST] = f; state[S_DENOM] = d; }
}

__device__ __forceinline__ double pg_block_max(double v, double *__restrict__ lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) lds[t] = fmax(lds[t], lds[t + h]);
        __syncthreads();
    }
    return lds[0];
}

// rules 1 and 2 of an attempt: the frozen row, and the gradient test
__global__ __launch_bounds__(256) void pg_gate_kernel(const double *__restrict__ bvec, int n, int attempt, double gradient_tolerance,
                                                      double *__restrict__ state, double *__restrict__ history) {
    __shared__ double lds[256];
    const bool frozen = state[S_STATUS] != 0.0;
    double m = 0.0;
    if (!frozen)
        for (int i = threadIdx.x; i < n; i += 256) m = fmax(m, fabs(bvec[i]));
    m = pg_block_max(m, lds);
    if (threadIdx.x != 0) return;
    double *row = history + (int64_t)attempt * PG_ROW;
    state[S_ACCEPTED] = 0.0;
    if (frozen) {
        state[S_LIVE] = 0.0;
        row[0] = state[S_COST]; row[1] = state[S_LAMBDA]; row[2] = 0.0; row[3] = 0.0; row[4] = 0.0; row[5] = 0.0;
        row[6] = state[S_STATUS]; row[7] = state[S_NU];
        return;
    }
    state[S_GMAX] = m;
    if (m < gradient_tolerance) {
        state[S_STATUS] = 1.0; state[S_LIVE] = 0.0;
        row[0] = state[S_COST]; row[1] = state[S_LAMBDA]; row[2] = 0.0; row[3] = m; row[4] = 0.0; row[5] = 0.0;
        row[6] = 1.0; row[7] = state[S_NU];
        return;
    }
    state[S_LIVE] = 1.0;
}

// one lane per node: P' = [dR(omega) | v] P
__global__ __launch_bounds__(256) void pg_trial_kernel(const double *__restrict__ poses, const double *__restrict__ delta, int N,
                                                       const double *__restrict__ state, double *__restrict__ trial) {
    if (state[S_STATUS] != 0.0) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double *P = poses + (int64_t)i * 16, *x = delta + (int64_t)i * 6;
    const double wx = x[0], wy = x[1], wz = x[2];
    const double v[3] = {x[3], x[4], x[5]};
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double a = 1.0, b = 0.5;
    if (!(th2 < PG_SMALL_THETA2)) {
        const double th = sqrt(th2);
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    const double R[9] = {1.0 + b * (wx * wx - th2), -(a * wz) + b * (wx * wy), a * wy + b * (wx * wz),
                         a * wz + b * (wx * wy), 1.0 + b * (wy * wy - th2), -(a * wx) + b * (wy * wz),
                         -(a * wy) + b * (wx * wz), a * wx + b * (wy * wz), 1.0 + b * (wz * wz - th2)};
    double *out = trial + (int64_t)i * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double t = (R[r * 3] * P[c] + R[r * 3 + 1] * P[4 + c]) + R[r * 3 + 2] * P[8 + c];
            if (c == 3) t += v[r];
            out[r * 4 + c] = t;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) out[12 + c] = P[12 + c];
}

// mode 0, the prologue: F, lambda = tau max_i H_ii over the free rows, nu = 2.  mode 1, rules 5 and 6 of an attempt; an accepted
// trial's poses and line weights are copied by the whole workgroup.
__global__ __launch_bounds__(256) void pg_decide_kernel(int mode, int attempt, const double *__restrict__ H, int n, int fixed,
                                                        double relative_cost, double *__restrict__ poses, const double *__restrict__ trial,
                                                        double *__restrict__ l, const double *__restrict__ l_trial, int N, int E,
                                                        double *__restrict__ state, double *__restrict__ history) {
    __shared__ double lds[256];
    __shared__ int take;
    const int t = threadIdx.x;
    if (mode == 0) {
        if (state[S_STATUS] != 0.0) return;
        double m = 0.0;
        for (int i = t; i < n; i += 256)
            if (i / 6 != fixed) m = fmax(m, H[(int64_t)i * n + i]);
        m = pg_block_max(m, lds);
        if (t == 0) {
            state[S_COST] = state[S_TRIAL_COST];
            state[S_LAMBDA] = PG_TAU * m;
            state[S_NU] = 2.0;
        }
        for (int e = t; e < E; e += 256) l[e] = l_trial[e];
        return;
    }
    if (state[S_LIVE] == 0.0) return;
    if (t == 0) {
        take = 0;
        double *row = history + (int64_t)attempt * PG_ROW;
        const double F = state[S_COST], lambda = state[S_LAMBDA], nu = state[S_NU];
        state[S_ATTEMPTS] += 1.0;
        if (state[S_STATUS] != 0.0) {                    // the solve met a failed pivot
            row[0] = F; row[1] = lambda; row[2] = 0.0; row[3] = state[S_GMAX]; row[4] = 0.0; row[5] = 0.0;
            row[6] = state[S_STATUS]; row[7] = nu;
        } else {
            const double Ft = state[S_TRIAL_COST], den = state[S_DENOM];
            double rho = 0.0, status = 0.0, Fn = F, ln = lambda, nn = nu;
            bool accept = false;
            if (finite_f64(den) && den > 0.0) {
                rho = (F - Ft) / den;
                accept = rho > 0.0;
            }
            if (accept) {
                const double s = 2.0 * rho - 1.0;
                ln = lambda * fmax(1.0 / 3.0, 1.0 - (s * s) * s);
                nn = 2.0;
                state[S_ITER] += 1.0;
                if (F - Ft <= relative_cost * F) status = 1.0;
                Fn = Ft;
                take = 1;
            } else if (fabs(F - Ft) <= relative_cost * F) {
                status = 1.0;                            // the trial's cost cannot be told from F: rounding decides rho, not the model
            } else {
                ln = lambda * nu;
                nn = 2.0 * nu;
                if (!finite_f64(ln)) status = 2.0;
            }
            state[S_COST] = Fn; state[S_LAMBDA] = ln; state[S_NU] = nn; state[S_STATUS] = status;
            state[S_ACCEPTED] = accept ? 1.0 : 0.0;
            row[0] = Fn; row[1] = ln; row[2] = rho; row[3] = state[S_GMAX]; row[4] = accept ? 1.0 : 0.0; row[5] = Ft;
            row[6] = status; row[7] = nn;
        }
    }
    __syncthreads();
    if (!take) return;
    for (int i = t; i < N * 16; i += 256) poses[i] = trial[i];
    for (int e = t; e < E; e += 256) l[e] = l_trial[e];
}

// ---------------------------------------------------------------- the dense SPD solve
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int SB = 64;            // panel width and tile edge
constexpr int SP = SB + 1;        // LDS row pitch of a 64 x 64 tile walked down its columns: (i * 65 + j) spreads a column over the banks
constexpr int SKS = 32, SKP = SKS + 2;   // K stage of the trailing update and its pitch: 16 rows x 2 k of 8 bytes land on 32 distinct slots

// W = A + lambda I on the lower tiles, the identity in the padding; d0 = the diagonal W starts from; y = b (0 in the padding)
__global__ __launch_bounds__(256) void spd_copy_kernel(const double *__restrict__ A, int n, int64_t ld, const double *__restrict__ lambda,
                                                       const double *__restrict__ b, double *__restrict__ W, int64_t np,
                                                       double *__restrict__ d0, double *__restrict__ y, const double *__restrict__ status) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti || *status != 0.0) return;
    const double lam = lambda ? *lambda : 0.0;
    for (int idx = threadIdx.x; idx < SB * SB; idx += 256) {
        const int64_t i = (int64_t)ti * SB + (idx >> 6), j = (int64_t)tj * SB + (idx & 63);
        double v = i == j ? 1.0 : 0.0;
        if (i < n && j < n) {
            v = A[i * ld + j];
            if (i == j) v = v + lam;
        }
        W[i * np + j] = v;
        if (i == j) {
            d0[i] = v;
            y[i] = i < n ? b[i] : 0.0;
        }
    }
}

// the diagonal tile k, in LDS, column by column; a failed pivot sets the status word and leaves the tile as it was
__global__ __launch_bounds__(256) void spd_diag_kernel(double *__restrict__ W, int64_t np, int k, const double *__restrict__ d0,
                                                       double *__restrict__ status) {
    __shared__ double S[SB][SP];
    if (*status != 0.0) return;
    const int tid = threadIdx.x;
    double *tile = W + ((int64_t)k * SB) * np + (int64_t)k * SB;
    for (int idx = tid; idx < SB * SB; idx += 256) S[idx >> 6][idx & 63] = tile[(int64_t)(idx >> 6) * np + (idx & 63)];
    const int i = tid & 63, cg = tid >> 6;
    for (int j = 0; j < SB; ++j) {
        __syncthreads();
        const double piv = S[j][j];
        if (!finite_f64(piv) || piv <= PG_PIVOT_REL * d0[k * SB + j]) {          // (the same for every lane)
            if (tid == 0) *status = 2.0;
            return;
        }
        const double d = sqrt(piv);
        __syncthreads();
        if (tid < SB && tid >= j) S[tid][j] = tid == j ? d : S[tid][j] / d;
        __syncthreads();
        const double lij = S[i][j];
        for (int c = j + 1 + cg; c <= i; c += 4) S[i][c] = __builtin_fma(-lij, S[c][j], S[i][c]);
    }
    __syncthreads();
    for (int idx = tid; idx < SB * SB; idx += 256) tile[(int64_t)(idx >> 6) * np + (idx & 63)] = S[idx >> 6][idx & 63];
}

// the tiles below the diagonal tile: X L_kk^T = W, one lane per row, the row in registers
__global__ __launch_bounds__(64) void spd_panel_kernel(double *__restrict__ W, int64_t np, int k, const double *__restrict__ status) {
    __shared__ double Ls[SB][SP];
    if (*status != 0.0) return;
    const int lane = threadIdx.x;
    const double *tile = W + ((int64_t)k * SB) * np + (int64_t)k * SB;
    for (int idx = lane; idx < SB * SB; idx += 64) Ls[idx >> 6][idx & 63] = tile[(int64_t)(idx >> 6) * np + (idx & 63)];
    __syncthreads();
    double *row = W + ((int64_t)(k + 1 + blockIdx.x) * SB + lane) * np + (int64_t)k * SB;
    double x[SB];
#pragma unroll
    for (int c = 0; c < SB; ++c) x[c] = row[c];
    // column c is finished, then taken out of every later column: x[j] meets its terms in ascending c, and the 63 - c updates of
    // a step do not wait for each other
#pragma unroll
    for (int c = 0; c < SB; ++c) {
        x[c] = x[c] / Ls[c][c];
#pragma unroll
        for (int j = c + 1; j < SB; ++j) x[j] = __builtin_fma(-x[c], Ls[j][c], x[j]);
    }
#pragma unroll
    for (int c = 0; c < SB; ++c) row[c] = x[c];
}

// the trailing tiles (ti >= tj > k): W_ij -= X_i X_j^T, four wavefronts of 32 x 32 (2 x 2 MFMA blocks), K in two stages of 32
__global__ __launch_bounds__(256) void spd_trail_kernel(double *__restrict__ W, int64_t np, int k, const double *__restrict__ status) {
    const int ti = k + 1 + blockIdx.y, tj = k + 1 + blockIdx.x;
    if (tj > ti || *status != 0.0) return;
    __shared__ double As[SB][SKP], Bs[SB][SKP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fk = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int ea = 0; ea < 2; ++ea)
#pragma unroll
        for (int eb = 0; eb < 2; ++eb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[ea][eb][r] = W[((int64_t)ti * SB + wm * 32 + ea * 16 + fk + 4 * r) * np + (int64_t)tj * SB + wn * 32 + eb * 16 + fr];
    const int sr = tid >> 2, sc = (tid & 3) * 8;
    for (int k0 = 0; k0 < SB; k0 += SKS) {
        __syncthreads();
        const double *pa = W + ((int64_t)ti * SB + sr) * np + (int64_t)k * SB + k0 + sc;
        const double *pb = W + ((int64_t)tj * SB + sr) * np + (int64_t)k * SB + k0 + sc;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            As[sr][sc + c] = -pa[c];
            Bs[sr][sc + c] = pb[c];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SKS / 4; ++s) {
            double a[2], b[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[e] = As[wm * 32 + e * 16 + fr][s * 4 + fk];
                b[e] = Bs[wn * 32 + e * 16 + fr][s * 4 + fk];
            }
#pragma unroll
            for (int ea = 0; ea < 2; ++ea)
#pragma unroll
                for (int eb = 0; eb < 2; ++eb) acc[ea][eb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ea = 0; ea < 2; ++ea)
#pragma unroll
        for (int eb = 0; eb < 2; ++eb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                W[((int64_t)ti * SB + wm * 32 + ea * 16 + fk + 4 * r) * np + (int64_t)tj * SB + wn * 32 + eb * 16 + fr] = acc[ea][eb][r];
}

// the 64 unknowns of block k from the diagonal tile, by one wavefront: forward L z = y, backward L^T x = z
template <bool FORWARD>
__device__ __forceinline__ void spd_tri_solve(const double (&Ls)[SB][SP], double *__restrict__ v) {
    const int lane = threadIdx.x;
    for (int s = 0; s < SB; ++s) {
        const int c = FORWARD ? s : SB - 1 - s;
        __syncthreads();
        if (lane == c) v[c] = v[c] / Ls[c][c];
        __syncthreads();
        if (FORWARD ? lane > c : lane < c) v[lane] = __builtin_fma(-(FORWARD ? Ls[lane][c] : Ls[c][lane]), v[c], v[lane]);
    }
    __syncthreads();
}

// substitution step k: every workgroup solves block k for itself; workgroup 0 stores it, workgroup j >= 1 takes it out of the
// right-hand side of one row block still to come (forward: block k + j, below; backward: block j - 1, above)
template <bool FORWARD>
__global__ __launch_bounds__(64) void spd_subst_kernel(const double *__restrict__ W, int64_t np, int k, double *__restrict__ rhs,
                                                       double *__restrict__ out, int64_t out_n, const double *__restrict__ status) {
    __shared__ double Ls[SB][SP];
    __shared__ double v[SB];
    if (*status != 0.0) return;
    const int lane = threadIdx.x;
    const double *tile = W + ((int64_t)k * SB) * np + (int64_t)k * SB;
    for (int idx = lane; idx < SB * SB; idx += 64) Ls[idx >> 6][idx & 63] = tile[(int64_t)(idx >> 6) * np + (idx & 63)];
    v[lane] = rhs[(int64_t)k * SB + lane];
    spd_tri_solve<FORWARD>(Ls, v);
    if (blockIdx.x == 0) {
        if ((int64_t)k * SB + lane < out_n) out[(int64_t)k * SB + lane] = v[lane];
        return;
    }
    const int64_t row = (int64_t)(FORWARD ? k + blockIdx.x : blockIdx.x - 1) * SB + lane;
    double t = rhs[row];
    if (FORWARD) {
        const double *p = W + row * np + (int64_t)k * SB;
        for (int c = 0; c < SB; ++c) t = __builtin_fma(-p[c], v[c], t);
    } else {
        const double *p = W + ((int64_t)k * SB) * np + row;
        for (int c = 0; c < SB; ++c) t = __builtin_fma(-p[(int64_t)c * np], v[c], t);
    }
    rhs[row] = t;
}

static inline int64_t spd_padded(int64_t n) { return (n + SB - 1) / SB * SB; }

}  // namespace

extern "C" int sgam_pose_graph_check(const int32_t *src_host, const int32_t *dst_host, int32_t E, int32_t N, int32_t fixed) {
    if (N < 1 || N > PG_MAX_NODES || E < 0 || E > PG_MAX_EDGES || fixed < 0 || fixed >= N || (E > 0 && (!src_host || !dst_host)))
        return SGAM_EINVAL;
    for (int32_t e = 0; e < E; ++e) {
        const int32_t s = src_host[e], t = dst_host[e];
        if (s < 0 || s >= N || t < 0 || t >= N || s == t) return SGAM_EINVAL;
    }
    return SGAM_OK;
}

extern "C" int sgam_pose_graph_linearize(const double *poses, int32_t N, const int32_t *src, const int32_t *dst, const double *transforms,
                                         const double *information, const uint8_t *uncertain, int32_t E, const double *state, double *r,
                                         double *J, double *q, double *l, double *cost, double *K, double *g, void *stream) {
    if (!poses || !src || !dst || !transforms || !information || !uncertain || !state || !r || !J || !q || !l || !cost || !K || !g ||
        N < 1 || N > PG_MAX_NODES || E < 1 || E > PG_MAX_EDGES)
        return SGAM_EINVAL;
    SGAM_KLAUNCH(pg_linearize_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, sgam_stream(stream), poses, src, dst, transforms,
                 information, uncertain, (int)E, state, r, J, q, l, cost, K, g);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_pose_graph_assemble(const double *K, const double *g, int32_t N, int32_t fixed, const int32_t *block_row,
                                        const int32_t *block_col, const int32_t *block_ptr, const int32_t *block_entry, int32_t blocks,
                                        const double *state, int32_t gated, double *H, double *b, void *stream) {
    if (!K || !g || !block_row || !block_col || !block_ptr || !block_entry || !state || !H || !b || N < 1 || N > PG_MAX_NODES || fixed < 0 ||
        fixed >= N || blocks < N || blocks > N + PG_MAX_EDGES)
        return SGAM_EINVAL;
    const int64_t count = (int64_t)N * 6 * N * 6;
    const unsigned grid = (unsigned)(count / 256 < 1 ? 1 : (count / 256 > 4096 ? 4096 : count / 256));
    SGAM_KLAUNCH(pg_zero_kernel, dim3(grid), dim3(256), 0, sgam_stream(stream), H, count, state, (int)gated);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(pg_gather_kernel, dim3((unsigned)blocks), dim3(64), 0, sgam_stream(stream), K, g, (int)N, (int)fixed, block_row, block_col,
                 block_ptr, block_entry, state, (int)gated, H, b);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_pose_graph_fold(const double *cost, int32_t E, const double *delta, const double *b, int32_t n, double *state,
                                    void *stream) {
    if (!cost || !state || E < 1 || E > PG_MAX_EDGES || (delta && (!b || n < 1 || n > SPD_MAX_N))) return SGAM_EINVAL;
    SGAM_KLAUNCH(pg_fold_kernel, dim3(1), dim3(256), 0, sgam_stream(stream), cost, (int)E, delta, b, (int)n, state);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_pose_graph_gate(const double *b, int32_t n, int32_t attempt, double gradient_tolerance, double *state, double *history,
                                    void *stream) {
    if (!b || !state || !history || n < 1 || n > SPD_MAX_N || attempt < 0 || !(gradient_tolerance >= 0.0)) return SGAM_EINVAL;
    SGAM_KLAUNCH(pg_gate_kernel, dim3(1), dim3(256), 0, sgam_stream(stream), b, (int)n, (int)attempt, gradient_tolerance, state, history);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_pose_graph_trial(const double *poses, const double *delta, int32_t N, const double *state, double *trial, void *stream) {
    if (!poses || !delta || !state || !trial || N < 1 || N > PG_MAX_NODES) return SGAM_EINVAL;
    SGAM_KLAUNCH(pg_trial_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), poses, delta, (int)N, state, trial);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_pose_graph_decide(int32_t mode, int32_t attempt, const double *H, int32_t N, int32_t fixed, double relative_cost,
                                      double *poses, const double *trial, double *l, const double *l_trial, int32_t E, double *state,
                                      double *history, void *stream) {
    if ((mode != 0 && mode != 1) || !l || !l_trial || !state || N < 1 || N > PG_MAX_NODES || E < 1 || E > PG_MAX_EDGES || fixed < 0 ||
        fixed >= N || (mode == 0 && !H) || (mode == 1 && (!poses || !trial || !history || attempt < 0 || !(relative_cost >= 0.0))))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(pg_decide_kernel, dim3(1), dim3(256), 0, sgam_stream(stream), (int)mode, (int)attempt, H, (int)N * 6, (int)fixed,
                 relative_cost, poses, trial, l, l_trial, (int)N, (int)E, state, history);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_spd_solve_workspace_doubles(int32_t n) {
    if (n < 1 || n > SPD_MAX_N) return SGAM_EINVAL;
    const int64_t np = spd_padded(n);
    return np * np + 3 * np;
}

extern "C" int sgam_spd_solve_f64(const double *A, int32_t n, int64_t ld, const double *lambda, const double *b, double *workspace,
                                  int64_t workspace_doubles, double *x, double *status, void *stream) {
    if (!A || !b || !workspace || !x || !status || n < 1 || n > SPD_MAX_N || ld < n || workspace_doubles < sgam_spd_solve_workspace_doubles(n))
        return SGAM_EINVAL;
    const int64_t np = spd_padded(n);
    const int T = (int)(np / SB);
    double *W = workspace, *d0 = W + np * np, *y = d0 + np, *z = y + np;
    hipStream_t st = sgam_stream(stream);
    SGAM_KLAUNCH(spd_copy_kernel, dim3(T, T), dim3(256), 0, st, A, (int)n, ld, lambda, b, W, np, d0, y, status);
    SGAM_LAUNCH_CHECK();
    for (int k = 0; k < T; ++k) {
        SGAM_KLAUNCH(spd_diag_kernel, dim3(1), dim3(256), 0, st, W, np, k, d0, status);
        SGAM_LAUNCH_CHECK();
        if (k + 1 < T) {
            SGAM_KLAUNCH(spd_panel_kernel, dim3(T - k - 1), dim3(64), 0, st, W, np, k, status);
            SGAM_LAUNCH_CHECK();
            SGAM_KLAUNCH(spd_trail_kernel, dim3(T - k - 1, T - k - 1), dim3(256), 0, st, W, np, k, status);
            SGAM_LAUNCH_CHECK();
        }
    }
    for (int k = 0; k < T; ++k) {
        SGAM_KLAUNCH(spd_subst_kernel<true>, dim3(T - k), dim3(64), 0, st, W, np, k, y, z, np, status);
        SGAM_LAUNCH_CHECK();
    }
    for (int k = T - 1; k >= 0; --k) {
        SGAM_KLAUNCH(spd_subst_kernel<false>, dim3(k + 1), dim3(64), 0, st, W, np, k, z, x, (int64_t)n, status);
        SGAM_LAUNCH_CHECK();
    }
    return SGAM_OK;
}
