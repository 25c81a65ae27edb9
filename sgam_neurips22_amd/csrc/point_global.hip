// point_global.hip — global registration of two clouds that share no frame, the stage before ICP (point_icp.hip): FPFH features
// (Rusu, Blodow, Beetz, ICRA 2009) from a cloud's k-NN rows and oriented normals (sgam_points_fpfh_counts,
// sgam_points_fpfh_combine_f32), the nearest feature by brute force (sgam_features_match_f32) and RANSAC over the feature
// correspondences: the hypotheses with their checks and Horn's closed-form pose (sgam_points_ransac_hypotheses), their inlier
// counts and the best of them (sgam_points_ransac_score), and the winner unpacked into the refit's fixed correspondences
// (sgam_points_ransac_inliers).  Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching as documented.
// Every rule — the pair features, the bins, the draw, the checks, the pose — is stated once in include/sgam_hip.h and restated in
// tests/global_registration_oracle.py; points_common.h's arithmetic rules hold: one IEEE operation per operator in the written
// order, integer atomics only, every output a function of the inputs only.  DESIGN §4.4.6.
//
// No transcendental decides a bin: theta = atan2(y, x) is never evaluated, its bin is counted from the signs of the cross
// products with the ten bin-edge directions below.  No kernel indexes a lane-private array by a run-time value (the histogram of
// a lane lives in LDS, the 4 x 4 eigen-solver is unrolled over its index pairs): no private memory.
#include "points_common.h"

#include <cmath>

namespace {

constexpr int FPFH_DIM = 33, FPFH_ROW = 34;   // counts per point; an int32 row of `counts`: the 33 and the number of pairs
constexpr int MATCH_TILE = 256;               // target rows staged per pass of the nearest-feature kernel
constexpr int MATCH_PITCH = 36;               // floats between two staged rows: 16-byte aligned rows, read four values at a time
constexpr int RANSAC_MAX_DRAWS = 16;          // Philox draws a hypothesis may use for its ransac_n distinct picks
constexpr int RANSAC_SWEEPS = 8;              // cyclic Jacobi sweeps over the 4 x 4 matrix of Horn's form (a fixed count)
constexpr int SCORE_TILE = 256;               // correspondences staged per pass of the scoring kernel

// the bin edges of theta: (cos, sin)(-pi + 2 pi b / 11), b = 1..10
constexpr double EC1 = -0.8412535328311811, ES1 = -0.5406408174555978;
constexpr double EC2 = -0.4154150130018863, ES2 = -0.9096319953545184;
constexpr double EC3 = 0.14231483827328512, ES3 = -0.9898214418809327;
constexpr double EC4 = 0.6548607339452851, ES4 = -0.7557495743542583;
constexpr double EC5 = 0.9594929736144975, ES5 = -0.2817325568414295;
constexpr double EC6 = 0.9594929736144975, ES6 = 0.2817325568414295;
constexpr double EC7 = 0.6548607339452851, ES7 = 0.7557495743542583;
constexpr double EC8 = 0.14231483827328512, ES8 = 0.9898214418809327;
constexpr double EC9 = -0.41541501300188616, ES9 = 0.9096319953545186;
constexpr double EC10 = -0.8412535328311813, ES10 = 0.5406408174555974;

__device__ __forceinline__ int past_edge(double c, double s, double x, double y) { return c * y - s * x >= 0.0 ? 1 : 0; }

__device__ __forceinline__ int theta_bin(double x, double y) {
    if (x == 0.0 && y == 0.0) return 5;
    if (y < 0.0)
        return past_edge(EC1, ES1, x, y) + past_edge(EC2, ES2, x, y) + past_edge(EC3, ES3, x, y) + past_edge(EC4, ES4, x, y) +
               past_edge(EC5, ES5, x, y);
    return 5 + past_edge(EC6, ES6, x, y) + past_edge(EC7, ES7, x, y) + past_edge(EC8, ES8, x, y) + past_edge(EC9, ES9, x, y) +
           past_edge(EC10, ES10, x, y);
}

__device__ __forceinline__ int unit_bin(double f) {
    const double t = floor((11.0 * (f + 1.0)) * 0.5);
    return t < 0.0 ? 0 : (t > 10.0 ? 10 : (int)t);
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// one lane per point; its 33 counters are a column of the LDS table (no other lane touches it: no barrier)
__global__ __launch_bounds__(256) void fpfh_counts_kernel(const float *__restrict__ points, const float *__restrict__ normals, int N,
                                                          const int32_t *__restrict__ knn_index, int k, int32_t *__restrict__ counts) {
    __shared__ int hist[FPFH_DIM][256];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + lane;
    if (i >= N) return;
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) hist[b][lane] = 0;
    const float fx = points[i * 3], fy = points[i * 3 + 1], fz = points[i * 3 + 2];
    const float hx = normals[i * 3], hy = normals[i * 3 + 1], hz = normals[i * 3 + 2];
    int m = 0;
    if (finite3(fx, fy, fz) && finite3(hx, hy, hz)) {
        const double px = (double)fx, py = (double)fy, pz = (double)fz, nix = (double)hx, niy = (double)hy, niz = (double)hz;
#pragma unroll 1
        for (int c = 0; c < k; ++c) {
            const int j = knn_index[i * k + c];
            if (j < 0 || j >= N || j == i) continue;
            const float gx = points[(int64_t)j * 3], gy = points[(int64_t)j * 3 + 1], gz = points[(int64_t)j * 3 + 2];
            const float ux = normals[(int64_t)j * 3], uy = normals[(int64_t)j * 3 + 1], uz = normals[(int64_t)j * 3 + 2];
            if (!finite3(gx, gy, gz) || !finite3(ux, uy, uz)) continue;
            double dx = (double)gx - px, dy = (double)gy - py, dz = (double)gz - pz;
            const double d = sqrt(dot3(dx, dy, dz, dx, dy, dz));
            if (d == 0.0) continue;
            const double njx = (double)ux, njy = (double)uy, njz = (double)uz;
            const double a1 = dot3(nix, niy, niz, dx, dy, dz) / d, a2 = dot3(njx, njy, njz, dx, dy, dz) / d;
            const bool swap = fabs(a1) < fabs(a2);
            const double n1x = swap ? njx : nix, n1y = swap ? njy : niy, n1z = swap ? njz : niz;
            const double n2x = swap ? nix : njx, n2y = swap ? niy : njy, n2z = swap ? niz : njz;
            const double f2 = swap ? -a2 : a1;
            if (swap) { dx = -dx; dy = -dy; dz = -dz; }
            double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
            const double vn = sqrt(dot3(vx, vy, vz, vx, vy, vz));
            if (vn == 0.0) continue;
            vx = vx / vn; vy = vy / vn; vz = vz / vn;
            const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
            const double f1 = dot3(vx, vy, vz, n2x, n2y, n2z);
            const double x = dot3(n1x, n1y, n1z, n2x, n2y, n2z), y = dot3(wx, wy, wz, n2x, n2y, n2z);
            hist[theta_bin(x, y)][lane] += 1;
            hist[11 + unit_bin(f1)][lane] += 1;
            hist[22 + unit_bin(f2)][lane] += 1;
            ++m;
        }
    }
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) counts[i * FPFH_ROW + b] = hist[b][lane];
    counts[i * FPFH_ROW + FPFH_DIM] = m;
}

// one lane per point; the 33 sums are indexed by unrolled loops only
__global__ __launch_bounds__(256) void fpfh_combine_kernel(const int32_t *__restrict__ counts, const float *__restrict__ points,
                                                           const float *__restrict__ normals, int N, const int32_t *__restrict__ knn_index,
                                                           const float *__restrict__ knn_d2, int k, float *__restrict__ features) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float *out = features + i * FPFH_DIM;
    if (!finite3(points[i * 3], points[i * 3 + 1], points[i * 3 + 2]) || !finite3(normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2])) {
        const float nanf_ = __uint_as_float(0x7fc00000u);
#pragma unroll
        for (int b = 0; b < FPFH_DIM; ++b) out[b] = nanf_;
        return;
    }
    double A[FPFH_DIM];
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) A[b] = 0.0;
#pragma unroll 1
    for (int c = 1; c < k; ++c) {
        const int j = knn_index[i * k + c];
        if (j < 0 || j >= N) continue;
        const float d2 = knn_d2[i * k + c];
        if (!(d2 > 0.0f) || !(d2 <= F32_MAX)) continue;
        const int32_t *row = counts + (int64_t)j * FPFH_ROW;
        const int mj = row[FPFH_DIM];
        if (mj <= 0) continue;
        const double scale = 100.0 / (double)mj, dd = (double)d2;
#pragma unroll
        for (int b = 0; b < FPFH_DIM; ++b) A[b] += ((double)row[b] * scale) / dd;
    }
    const int32_t *own = counts + i * FPFH_ROW;
    const int mi = own[FPFH_DIM];
    const double own_scale = mi > 0 ? 100.0 / (double)mi : 0.0;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        double S = A[f * 11];
#pragma unroll
        for (int b = 1; b < 11; ++b) S += A[f * 11 + b];
#pragma unroll
        for (int b = 0; b < 11; ++b) {
            const double spfh = (double)own[f * 11 + b] * own_scale;
            out[f * 11 + b] = (float)(S == 0.0 ? spfh : (100.0 * A[f * 11 + b]) / S + spfh);
        }
    }
}

// one lane per source row, its D values in registers; the target rows pass through LDS, every lane reading the same address
template <int D>
__global__ __launch_bounds__(256) void match_kernel(const float *__restrict__ source, int Ns, const float *__restrict__ target, int Nt,
                                                    float *__restrict__ d2_out, int32_t *__restrict__ index_out) {
    __shared__ __align__(16) float tile[MATCH_TILE * MATCH_PITCH];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + lane;
    float q[D];
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = i < Ns ? source[i * D + j] : 0.0f;
    float best = __uint_as_float(0x7f800000u);
    int best_index = -1;
    for (int base = 0; base < Nt; base += MATCH_TILE) {
        const int rows = min(MATCH_TILE, Nt - base);
        __syncthreads();
        for (int e = lane; e < rows * D; e += 256) {
            const int r = e / D;
            tile[r * MATCH_PITCH + (e - r * D)] = target[(int64_t)base * D + e];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const float *t = tile + r * MATCH_PITCH;
            float d = __fsub_rn(q[0], t[0]);
            float acc = __fmul_rn(d, d);
#pragma unroll
            for (int j = 1; j < D; ++j) {
                d = __fsub_rn(q[j], t[j]);
                acc = __fadd_rn(acc, __fmul_rn(d, d));
            }
            if (acc < best) { best = acc; best_index = base + r; }            // (ascending rows: a tie keeps the lower index)
        }
    }
    if (i < Ns) { d2_out[i] = best; index_out[i] = best_index; }
}

// one Jacobi rotation of the symmetric 4 x 4 A that zeroes A[P][Q], and of the eigenvector columns P, Q of V: point_cloud.hip's
// jacobi_rotate with two further rows
template <int P, int Q>
__device__ __forceinline__ void rotate4(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        const double pr = A[P][r], qr = A[Q][r];
        A[P][r] = c * pr - s * qr; A[r][P] = A[P][r];
        A[Q][r] = s * pr + c * qr; A[r][Q] = A[Q][r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double a = V[r][P], b = V[r][Q];
        V[r][P] = c * a - s * b;
        V[r][Q] = s * a + c * b;
    }
}

// one lane per hypothesis; NS = ransac_n.  Everything indexed by a slot is unrolled.
template <int NS>
__global__ __launch_bounds__(256) void ransac_hypotheses_kernel(const float *__restrict__ source, int Ns, const float *__restrict__ target, int Nt,
                                                                const int32_t *__restrict__ corr, int C, int H, double similarity,
                                                                double max_distance, uint32_t seed_lo, uint32_t seed_hi,
                                                                int32_t *__restrict__ samples, int32_t *__restrict__ valid,
                                                                double *__restrict__ poses) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    int pick[4] = {-1, -1, -1, -1};
    int draws = 0;
    bool ok = true;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        int got = -1;
        while (draws < RANSAC_MAX_DRAWS) {
            uint32_t w[4] = {(uint32_t)h, (uint32_t)draws, 0u, 0u};
            sgam_philox4x32_10(w, seed_lo, seed_hi);
            ++draws;
            const int cand = (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)C) >> 32);
            bool dup = false;
#pragma unroll
            for (int t = 0; t < s; ++t) dup = dup || pick[t] == cand;
            if (!dup) { got = cand; break; }
        }
        pick[s] = got;
        ok = ok && got >= 0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) samples[h * 4 + s] = pick[s];
    double p[NS][3], q[NS][3];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { p[s][a] = 0.0; q[s][a] = 0.0; }
        if (!ok) continue;
        const int si = corr[(int64_t)pick[s] * 2], ti = corr[(int64_t)pick[s] * 2 + 1];
        if (si < 0 || si >= Ns || ti < 0 || ti >= Nt) { ok = false; continue; }
        const float sx = source[(int64_t)si * 3], sy = source[(int64_t)si * 3 + 1], sz = source[(int64_t)si * 3 + 2];
        const float tx = target[(int64_t)ti * 3], ty = target[(int64_t)ti * 3 + 1], tz = target[(int64_t)ti * 3 + 2];
        if (!finite3(sx, sy, sz) || !finite3(tx, ty, tz)) { ok = false; continue; }
        p[s][0] = (double)sx; p[s][1] = (double)sy; p[s][2] = (double)sz;
        q[s][0] = (double)tx; q[s][1] = (double)ty; q[s][2] = (double)tz;
    }
    // 1. the edge lengths of the two sides agree
#pragma unroll
    for (int b = 1; b < NS; ++b) {
#pragma unroll
        for (int a = 0; a < b; ++a) {
            const double ax = p[a][0] - p[b][0], ay = p[a][1] - p[b][1], az = p[a][2] - p[b][2];
            const double bx = q[a][0] - q[b][0], by = q[a][1] - q[b][1], bz = q[a][2] - q[b][2];
            const double la = sqrt(dot3(ax, ay, az, ax, ay, az)), lb = sqrt(dot3(bx, by, bz, bx, by, bz));
            ok = ok && la >= similarity * lb && lb >= similarity * la;
        }
    }
    double pose[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) pose[e] = 0.0;
    if (ok) {
        // 2. Horn's closed form
        double cs[3], ct[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double u = p[0][a] + p[1][a], v = q[0][a] + q[1][a];
#pragma unroll
            for (int s = 2; s < NS; ++s) { u += p[s][a]; v += q[s][a]; }
            cs[a] = u / (double)NS;
            ct[a] = v / (double)NS;
        }
        double S[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                double u = (p[0][a] - cs[a]) * (q[0][b] - ct[b]);
#pragma unroll
                for (int s = 1; s < NS; ++s) u += (p[s][a] - cs[a]) * (q[s][b] - ct[b]);
                S[a][b] = u;
            }
        }
        double A[4][4], V[4][4];
        A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
        A[0][1] = S[1][2] - S[2][1]; A[0][2] = S[2][0] - S[0][2]; A[0][3] = S[0][1] - S[1][0];
        A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
        A[1][2] = S[0][1] + S[1][0]; A[1][3] = S[2][0] + S[0][2];
        A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
        A[2][3] = S[1][2] + S[2][1];
        A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b < a) A[a][b] = A[b][a];
                V[a][b] = a == b ? 1.0 : 0.0;
            }
        }
#pragma unroll 1
        for (int sweep = 0; sweep < RANSAC_SWEEPS; ++sweep) {
            rotate4<0, 1>(A, V); rotate4<0, 2>(A, V); rotate4<0, 3>(A, V);
            rotate4<1, 2>(A, V); rotate4<1, 3>(A, V); rotate4<2, 3>(A, V);
        }
        // the eigenvector of the largest eigenvalue (the lowest index on a tie): selects of values, nothing indexed
        double big = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
        for (int e = 1; e < 4; ++e) {
            if (A[e][e] > big) { big = A[e][e]; qw = V[0][e]; qx = V[1][e]; qy = V[2][e]; qz = V[3][e]; }
        }
        const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        qw = qw / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
        pose[0] = 1.0 - 2.0 * (qy * qy + qz * qz); pose[1] = 2.0 * (qx * qy - qw * qz); pose[2] = 2.0 * (qx * qz + qw * qy);
        pose[4] = 2.0 * (qx * qy + qw * qz); pose[5] = 1.0 - 2.0 * (qx * qx + qz * qz); pose[6] = 2.0 * (qy * qz - qw * qx);
        pose[8] = 2.0 * (qx * qz - qw * qy); pose[9] = 2.0 * (qy * qz + qw * qx); pose[10] = 1.0 - 2.0 * (qx * qx + qy * qy);
#pragma unroll
        for (int r = 0; r < 3; ++r) pose[r * 4 + 3] = ct[r] - dot3(pose[r * 4], pose[r * 4 + 1], pose[r * 4 + 2], cs[0], cs[1], cs[2]);
#pragma unroll
        for (int e = 0; e < 12; ++e) ok = ok && finite_f64(pose[e]);
        // 3. every sample lands within the distance
        const double limit = max_distance * max_distance;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double e2[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                e2[r] = (dot3(pose[r * 4], pose[r * 4 + 1], pose[r * 4 + 2], p[s][0], p[s][1], p[s][2]) + pose[r * 4 + 3]) - q[s][r];
            ok = ok && dot3(e2[0], e2[1], e2[2], e2[0], e2[1], e2[2]) <= limit;
        }
    }
    valid[h] = ok ? 1 : 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) poses[h * 12 + e] = ok ? pose[e] : 0.0;
}

// the valid hypotheses gathered into list[0 .. *n_list): counts of the others are written here
__global__ __launch_bounds__(256) void ransac_compact_kernel(const int32_t *__restrict__ valid, int H, int32_t *__restrict__ n_list,
                                                             int32_t *__restrict__ list, int32_t *__restrict__ counts) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    if (valid[h] != 0) list[atomicAdd(n_list, 1)] = (int)h;
    else counts[h] = -1;
}

// the six floats of correspondence c (source point, target point), NaN where it names no pair of points
__device__ __forceinline__ void pair_of(const float *__restrict__ source, int Ns, const float *__restrict__ target, int Nt,
                                        const int32_t *__restrict__ corr, int64_t c, float (&v)[6], int &si, int &ti) {
    const float nanf_ = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int e = 0; e < 6; ++e) v[e] = nanf_;
    si = corr[c * 2]; ti = corr[c * 2 + 1];
    if (si < 0 || si >= Ns || ti < 0 || ti >= Nt) return;
#pragma unroll
    for (int e = 0; e < 3; ++e) { v[e] = source[(int64_t)si * 3 + e]; v[3 + e] = target[(int64_t)ti * 3 + e]; }
}

__device__ __forceinline__ bool is_inlier(const float (&T)[12], float sx, float sy, float sz, float tx, float ty, float tz, float max_d2) {
    float X, Y, Z;
    transform34(T, sx, sy, sz, X, Y, Z);
    return dist2(X, Y, Z, tx, ty, tz) <= max_d2;                              // (a NaN is no inlier)
}

// one lane per hypothesis (of the list, or of all H); the correspondences pass through LDS, every lane reading the same address
__global__ __launch_bounds__(256) void ransac_score_kernel(const float *__restrict__ source, int Ns, const float *__restrict__ target, int Nt,
                                                           const int32_t *__restrict__ corr, int C, const double *__restrict__ poses,
                                                           const int32_t *__restrict__ valid, int H, float max_d2,
                                                           const int32_t *__restrict__ n_list, const int32_t *__restrict__ list,
                                                           int32_t *__restrict__ counts, unsigned long long *__restrict__ best) {
    __shared__ float pts[SCORE_TILE][6];
    const int lane = threadIdx.x;
    const int n = list ? min(*n_list, H) : H;
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + lane;
    if ((int64_t)blockIdx.x * blockDim.x >= n) return;                        // (the whole workgroup)
    const int h = slot < n ? (list ? list[slot] : (int)slot) : -1;
    const bool live = h >= 0 && h < H && valid[h] != 0;
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = live ? (float)poses[(int64_t)h * 12 + e] : 0.0f;
    int count = 0;
    for (int base = 0; base < C; base += SCORE_TILE) {
        const int rows = min(SCORE_TILE, C - base);
        __syncthreads();
        if (lane < rows) {
            float v[6];
            int si, ti;
            pair_of(source, Ns, target, Nt, corr, (int64_t)base + lane, v, si, ti);
#pragma unroll
            for (int e = 0; e < 6; ++e) pts[lane][e] = v[e];
        }
        __syncthreads();
        if (live) {
            for (int r = 0; r < rows; ++r)
                count += is_inlier(T, pts[r][0], pts[r][1], pts[r][2], pts[r][3], pts[r][4], pts[r][5], max_d2) ? 1 : 0;
        }
    }
    if (h >= 0 && h < H) {
        counts[h] = live ? count : -1;
        if (live) atomicMax(best, ((unsigned long long)(uint32_t)count << 32) | (unsigned long long)(0xffffffffu - (uint32_t)h));
    }
}

// one lane per correspondence
__global__ __launch_bounds__(256) void ransac_inliers_kernel(const float *__restrict__ source, int Ns, const float *__restrict__ target, int Nt,
                                                             const int32_t *__restrict__ corr, int C, const double *__restrict__ poses, int H,
                                                             const unsigned long long *__restrict__ best, float max_d2,
                                                             uint8_t *__restrict__ mask, int32_t *__restrict__ index, double *__restrict__ state,
                                                             int32_t *__restrict__ info) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long packed = best[0];
    const uint32_t h = 0xffffffffu - (uint32_t)(packed & 0xffffffffull);
    const bool none = packed == 0ull || h >= (uint32_t)H;
    if (c == 0) {
        info[0] = none ? -1 : (int)h;
        info[1] = none ? 0 : (int)(packed >> 32);
        if (!none) {
#pragma unroll
            for (int e = 0; e < 12; ++e) state[e] = poses[(int64_t)h * 12 + e];
            state[12] = 0.0; state[13] = 0.0; state[14] = 0.0; state[15] = 1.0;
        }
    }
    if (c >= C) return;
    bool in = false;
    if (!none) {
        float T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = (float)poses[(int64_t)h * 12 + e];
        float v[6];
        int si, ti;
        pair_of(source, Ns, target, Nt, corr, c, v, si, ti);
        in = is_inlier(T, v[0], v[1], v[2], v[3], v[4], v[5], max_d2);
        if (in) atomicMax(index + si, ti);                                    // (an inlier's rows are in range: its points are finite)
    }
    mask[c] = in ? 1 : 0;
}

bool cloud_args(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C) {
    return source && target && corr && Ns >= 1 && Nt >= 1 && C >= 1;
}

}  // namespace

extern "C" int sgam_points_fpfh_counts(const float *points, const float *normals, int32_t N, const int32_t *knn_index, int32_t k,
                                       int32_t *counts, void *stream) {
    if (!points || !normals || !knn_index || !counts || N < 1 || k < 1 || k > KNN_MAX_K) return SGAM_EINVAL;
    SGAM_KLAUNCH(fpfh_counts_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), points, normals, N, knn_index, k, counts);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_fpfh_combine_f32(const int32_t *counts, const float *points, const float *normals, int32_t N,
                                            const int32_t *knn_index, const float *knn_d2, int32_t k, float *features, void *stream) {
    if (!counts || !points || !normals || !knn_index || !knn_d2 || !features || N < 1 || k < 1 || k > KNN_MAX_K) return SGAM_EINVAL;
    SGAM_KLAUNCH(fpfh_combine_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), counts, points, normals, N, knn_index, knn_d2, k,
                 features);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_features_match_f32(const float *source, int32_t Ns, const float *target, int32_t Nt, int32_t dim, float *d2,
                                       int32_t *index, void *stream) {
    if (!source || !target || !d2 || !index || Ns < 1 || Nt < 1 || dim != FPFH_DIM) return SGAM_EINVAL;
    SGAM_KLAUNCH(match_kernel<FPFH_DIM>, dim3(blocks_of(Ns)), dim3(256), 0, sgam_stream(stream), source, Ns, target, Nt, d2, index);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_ransac_hypotheses(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C,
                                             int32_t H, int32_t ransac_n, double edge_length_similarity, double max_distance, uint64_t seed,
                                             int32_t *samples, int32_t *valid, double *poses, void *stream) {
    if (!cloud_args(source, Ns, target, Nt, corr, C) || !samples || !valid || !poses || H < 1 || (ransac_n != 3 && ransac_n != 4) ||
        !(edge_length_similarity >= 0.0 && edge_length_similarity <= 1.0) || !(max_distance > 0.0 && finite_f64(max_distance)))
        return SGAM_EINVAL;
    const uint32_t lo = (uint32_t)(seed & 0xffffffffull), hi = (uint32_t)(seed >> 32);
    if (ransac_n == 3)
        SGAM_KLAUNCH(ransac_hypotheses_kernel<3>, dim3(blocks_of(H)), dim3(256), 0, sgam_stream(stream), source, Ns, target, Nt, corr, C, H,
                     edge_length_similarity, max_distance, lo, hi, samples, valid, poses);
    else
        SGAM_KLAUNCH(ransac_hypotheses_kernel<4>, dim3(blocks_of(H)), dim3(256), 0, sgam_stream(stream), source, Ns, target, Nt, corr, C, H,
                     edge_length_similarity, max_distance, lo, hi, samples, valid, poses);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

// [0, 16): the list's length (an int32);  [16, 16 + r16(4 H)): the list
extern "C" int64_t sgam_points_ransac_score_workspace_bytes(int32_t H) {
    if (H < 1) return SGAM_EINVAL;
    return 16 + r16(4 * (int64_t)H);
}

extern "C" int sgam_points_ransac_score(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C,
                                        const double *poses, const int32_t *valid, int32_t H, float max_d2, int32_t compact, void *workspace,
                                        int64_t workspace_bytes, int32_t *counts, uint64_t *best, void *stream) {
    if (!cloud_args(source, Ns, target, Nt, corr, C) || !poses || !valid || !counts || !best || H < 1 || !(max_d2 >= 0.0f)) return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_points_ransac_score_workspace_bytes(H))) return SGAM_EWORKSPACE;
    hipStream_t st = sgam_stream(stream);
    int32_t *n_list = (int32_t *)workspace, *list = (int32_t *)((char *)workspace + 16);
    unsigned long long *best_ = (unsigned long long *)best;
    SGAM_KLAUNCH(fill_kernel<unsigned long long>, dim3(1), dim3(256), 0, st, best_, (int64_t)1, 0ull);
    if (compact) {
        SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(1), dim3(256), 0, st, n_list, (int64_t)1, (int32_t)0);
        SGAM_KLAUNCH(ransac_compact_kernel, dim3(blocks_of(H)), dim3(256), 0, st, valid, H, n_list, list, counts);
    }
    SGAM_KLAUNCH(ransac_score_kernel, dim3(blocks_of(H)), dim3(256), 0, st, source, Ns, target, Nt, corr, C, poses, valid, H, max_d2,
                 compact ? n_list : (const int32_t *)nullptr, compact ? list : (const int32_t *)nullptr, counts, best_);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_ransac_inliers(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C,
                                          const double *poses, int32_t H, const uint64_t *best, float max_d2, uint8_t *mask, int32_t *index,
                                          double *state, int32_t *info, void *stream) {
    if (!cloud_args(source, Ns, target, Nt, corr, C) || !poses || !best || !mask || !index || !state || !info || H < 1 || !(max_d2 >= 0.0f))
        return SGAM_EINVAL;
    hipStream_t st = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(blocks_of(Ns)), dim3(256), 0, st, index, (int64_t)Ns, (int32_t)-1);
    SGAM_KLAUNCH(ransac_inliers_kernel, dim3(blocks_of(C)), dim3(256), 0, st, source, Ns, target, Nt, corr, C, poses, H,
                 (const unsigned long long *)best, max_d2, mask, index, state, info);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
