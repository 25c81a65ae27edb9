// rgbd_odometry.hip — direct (image-space) RGB-D odometry of P frame pairs in lock step: the step that MINIMISES the reprojection
// error view_consistency.hip measures.  The pose of a pair (source camera -> target camera) is refined by Gauss-Newton steps on a
// photometric and a geometric residual of the pixels both frames see; the correspondence of a source pixel is its projection, the
// image gradients are the exact derivatives of the bilinear interpolant view_consistency evaluates.  Poses, stop state and history
// of every pair live on the device: an iteration of ALL pairs is two launches (accumulate, update) and reads nothing back.  The rule
// is stated step by step in include/sgam_hip.h and restated in numpy by tests/odometry_oracle.py; DESIGN §4.4.13.
//
// Pyramid (rgbd_pyramid_*_kernel): one lane per output pixel of a level, all F frames in one launch per level.
//   level 0:    I = (float)(r + g + b) / 765.0f (the sum an integer, one fp32 division), D = the stored depth, copied
//   level l+1:  rows r_k = clamp(2 i + k - 1, 0, H_l - 1), columns c_k = clamp(2 j + k - 1, 0, W_l - 1), k = 0, 1, 2
//               h(r) = (I[r][c_0] + 2.0f * I[r][c_1]) + I[r][c_2]       I' = ((h(r_0) + 2.0f * h(r_1)) + h(r_2)) * 0.0625f
//               D' = D[2 i][2 j]: no filtering, validity is never averaged.  Sizes (H_l + 1) / 2, (W_l + 1) / 2.
//
// Accumulate (rgbd_accumulate_kernel<INFO>): grid (workgroups over chunks of ODO_CHUNK = 1024 source pixels, P); a lane takes the
// pixels base + c * 256 + lane in ascending c, so the source reads coalesce; pairs[p], the four plane addresses and the pose
// state[p][0..11] (rounded to fp32 once) are wave-uniform loads.  The geometry of a pixel is view_consistency's, expression for
// expression (valid, pixel_ray, transform34, u, v, floorf, the corners, the class tests with tau = max_depth_diff); only class 6
// pixels contribute.  The four target depths, the four target intensities and the source intensity are requested together before
// the classification, which is written as selects.  Then, in fp64 on the widened fp32 values (wx, wy, X, Y, Z, the
// corners), one IEEE operation per operator:
//   L(c)   = top + wy * (bot - top),  top = c00 + wx * (c01 - c00),  bot = c10 + wx * (c11 - c10)
//   L_u(c) = (c01 - c00) + wy * ((c11 - c10) - (c01 - c00))            L_v(c) = bot - top
//   iz = 1.0 / Z;  ux = fx * iz;  uz = -((ux * X) * iz);  vy = fy * iz;  vz = -((vy * Y) * iz)          (du = (ux, 0, uz), dv = (0, vy, vz))
//   photometric:  g = (-(L_u(I) * ux), -(L_v(I) * vy), -(L_u(I) * uz + L_v(I) * vz));  r_I = sp * (I_s - L(I))
//   geometric:    g = (-(L_u(D) * ux), -(L_v(D) * vy), 1.0 - (L_u(D) * uz + L_v(D) * vz));  r_Z = sg * (Z - L(D))
//   either row:   c = (Y g.z - Z g.y,  Z g.x - X g.z,  X g.y - Y g.x);  J = w * (c.x, c.y, c.z, g.x, g.y, g.z), w = sp or sg
//   sg = sqrt(lambda_geometric), sp = sqrt(1.0 - lambda_geometric).
// The 32 slots of sgam_points_icp_accumulate: 0..20 J^T J (the photometric row's product, then the geometric row's, added), 21..26
// J^T r, 27 r_I^2 + r_Z^2, 28 (Z - L(D))^2 unweighted, 29 the covisible count, 30 the source pixels of class != 0, 31 zero.
// INFO (the information matrix of a pose-graph edge, the same kernel): q = p' for frames == NULL, else transform34(frames[p], p')
// in fp32; slots 0..20 are the point-to-point sums of sgam_points_icp_accumulate on q (G = [-[q]x | I]), 21..28 zero, 29..31 as above.
// Workgroup sums go to workspace [P][blocks][32] (block_sum_f64); no atomics.  In a step a pair that is frozen (status 2, or status
// 1 unless this is the first iteration of a level) reads nothing and gets zero sums, which the update does not look at.
//
// Update (rgbd_update_kernel): one workgroup of 64 lanes per pair.  Lane s < 32 folds slot s over the pair's workgroups in block
// order from 0.0 (equal bits run to run), written to sums[p] when asked for; lane 0 then applies rules 1-6 of
// sgam_points_icp_update (point_icp.hip), restated here word for word on state[p][24] and history[p][row], with one addition for
// the pyramid: on the first iteration of a level a status 1 returns to 0 before rule 1 and the stop test of rule 4 is skipped.
#include "points_common.h"

#include <cmath>

namespace {

constexpr int ODO_SLOTS = 32;
constexpr int ODO_PER_LANE = 4;                       // pixels a lane sums before the workgroup reduction of the 32 slots
constexpr int ODO_CHUNK = 256 * ODO_PER_LANE;
constexpr int ODO_MAX_LEVELS = 4;
constexpr int ODO_STATE = 24, ODO_ROW = 8;
constexpr double ODO_PIVOT_REL = 1e-12;               // point_icp.hip's ICP_PIVOT_REL and ICP_SMALL_THETA2
constexpr double ODO_SMALL_THETA2 = 1e-16;

struct OdoView {
    float kinv[9];                                    // the level's intrinsics, inverted in float64 and rounded once (host)
    float fx, fy, cx, cy, zn, zf, tau;
    int H, W, F;
};

__device__ __forceinline__ bool depth_valid(float x, float zn, float zf) { return fabsf(x) <= F32_MAX && zn <= x && x <= zf; }

static inline int64_t chunks_of(int64_t hw) { return (hw + ODO_CHUNK - 1) / ODO_CHUNK; }

// level 0: one lane per pixel of every frame; intensity, depth [F][H][W]
__global__ __launch_bounds__(256) void rgbd_pyramid_base_kernel(const float *const *__restrict__ depth_ptrs,
                                                                const uint8_t *const *__restrict__ rgb_ptrs, int64_t hw, int64_t n,
                                                                float *__restrict__ intensity, float *__restrict__ depth) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t f = k / hw, q = k - f * hw;
    const uint8_t *__restrict__ c = rgb_ptrs[f] + q * 3;
    intensity[k] = __fdiv_rn((float)((int)c[0] + (int)c[1] + (int)c[2]), 765.0f);
    depth[k] = depth_ptrs[f][q];
}

// level l -> l + 1: one lane per output pixel of every frame
__global__ __launch_bounds__(256) void rgbd_pyramid_down_kernel(const float *__restrict__ I, const float *__restrict__ D, int H, int W,
                                                                int Ho, int Wo, int64_t n, float *__restrict__ Io, float *__restrict__ Do) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t how = (int64_t)Ho * Wo;
    const int64_t f = k / how, q = k - f * how;
    const int i = (int)(q / Wo), j = (int)(q - (int64_t)i * Wo);
    const float *__restrict__ src = I + f * H * W;
    int r[3], c[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        r[t] = min(max(2 * i + t - 1, 0), H - 1);
        c[t] = min(max(2 * j + t - 1, 0), W - 1);
    }
    float v[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) v[a][b] = src[(int64_t)r[a] * W + c[b]];
    float h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) h[a] = __fadd_rn(__fadd_rn(v[a][0], __fmul_rn(2.0f, v[a][1])), v[a][2]);
    Io[k] = __fmul_rn(__fadd_rn(__fadd_rn(h[0], __fmul_rn(2.0f, h[1])), h[2]), 0.0625f);
    Do[k] = D[f * H * W + (int64_t)(2 * i) * W + 2 * j];                   // 2 i <= H - 1, 2 j <= W - 1 by the sizes
}

// one row of the normal equations into the slots (point_icp.hip's add_row)
__device__ __forceinline__ void add_row(double (&s)[ODO_SLOTS], const double (&J)[6], double r) {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = a; b < 6; ++b) s[k++] += J[a] * J[b];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) s[21 + a] += J[a] * r;
    s[27] += r * r;
}

// J = w * (p x g, g) of one residual with the gradient g with respect to the moved point p = (X, Y, Z)
__device__ __forceinline__ void row_of(double w, double X, double Y, double Z, double gx, double gy, double gz, double (&J)[6]) {
    J[0] = w * (Y * gz - Z * gy); J[1] = w * (Z * gx - X * gz); J[2] = w * (X * gy - Y * gx);
    J[3] = w * gx; J[4] = w * gy; J[5] = w * gz;
}

// grid (chunks of the level's H W source pixels, P); partial [P][gridDim.x][32]
template <bool INFO>
__global__ __launch_bounds__(256) void rgbd_accumulate_kernel(OdoView V, const float *const *__restrict__ depth_ptrs,
                                                              const float *const *__restrict__ inten_ptrs, const int32_t *__restrict__ pairs,
                                                              const double *__restrict__ state, const float *__restrict__ frames, double lambda,
                                                              int level_first, double *__restrict__ partial) {
    const int64_t hw = (int64_t)V.H * V.W;
    const int p = blockIdx.y;
    const int s = pairs[2 * p], t = pairs[2 * p + 1];                          // wave-uniform
    const double *__restrict__ st = state + (int64_t)p * ODO_STATE;
    const double status = st[18];
    const bool running = INFO || status == 0.0 || (status == 1.0 && level_first != 0);
    const bool pair_ok = running && s >= 0 && s < V.F && t >= 0 && t < V.F;    // (a bad or frozen pair reads nothing)
    const float *__restrict__ depth_s = pair_ok ? depth_ptrs[s] : nullptr, *__restrict__ depth_t = pair_ok ? depth_ptrs[t] : nullptr;
    const float *__restrict__ inten_s = pair_ok ? inten_ptrs[s] : nullptr, *__restrict__ inten_t = pair_ok ? inten_ptrs[t] : nullptr;
    float T[12], Fr[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = (float)st[k];
    const bool framed = INFO && frames != nullptr;
#pragma unroll
    for (int k = 0; k < 12; ++k) Fr[k] = framed ? frames[(int64_t)p * 12 + k] : 0.0f;
    const double sg = sqrt(lambda), sp = sqrt(1.0 - lambda);
    const double fx = (double)V.fx, fy = (double)V.fy;
    double sum[ODO_SLOTS];
#pragma unroll
    for (int k = 0; k < ODO_SLOTS; ++k) sum[k] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * ODO_CHUNK;
    for (int c = 0; c < ODO_PER_LANE; ++c) {
        const int64_t q = base + c * 256 + threadIdx.x;
        if (q >= hw || !pair_ok) break;
        const int i = (int)(q / V.W), j = (int)(q - (int64_t)i * V.W);
        const float d = depth_s[q];
        if (!depth_valid(d, V.zn, V.zf)) continue;
        sum[30] += 1.0;
        float a, b, cc, X, Y, Z;
        pixel_ray(V.kinv, i, j, a, b, cc);
        transform34(T, __fmul_rn(a, d), __fmul_rn(b, d), __fmul_rn(cc, d), X, Y, Z);
        const float u = __fadd_rn(__fdiv_rn(__fmul_rn(V.fx, X), Z), V.cx);
        const float v = __fadd_rn(__fdiv_rn(__fmul_rn(V.fy, Y), Z), V.cy);
        const float x0f = floorf(u), y0f = floorf(v);
        if (!(V.zn <= Z && Z <= V.zf && 0.0f <= x0f && x0f <= (float)(V.W - 2) && 0.0f <= y0f && y0f <= (float)(V.H - 2))) continue;
        const float wxf = __fsub_rn(u, x0f), wyf = __fsub_rn(v, y0f);
        const int x0 = (int)x0f, y0 = (int)y0f;                                // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2
        const int64_t o = (int64_t)y0 * V.W + x0;                              // o + W + 1 <= H W - 1
        const float *__restrict__ dt = depth_t + o, *__restrict__ it = inten_t + o;
        // every gather of the pixel, requested before anything looks at a value
        const float D00 = dt[0], D01 = dt[1], D10 = dt[V.W], D11 = dt[V.W + 1];
        const float I00 = it[0], I01 = it[1], I10 = it[V.W], I11 = it[V.W + 1];
        const float Is = inten_s[q];
        // the classification, as selects
        const bool right = wxf >= 0.5f, down = wyf >= 0.5f;
        const float Dn = down ? (right ? D11 : D10) : (right ? D01 : D00);
        const float e = __fsub_rn(Z, Dn);
        const bool all_ok = depth_valid(D00, V.zn, V.zf) && depth_valid(D01, V.zn, V.zf) && depth_valid(D10, V.zn, V.zf) &&
                            depth_valid(D11, V.zn, V.zf) && fabsf(__fsub_rn(Z, D00)) <= V.tau && fabsf(__fsub_rn(Z, D01)) <= V.tau &&
                            fabsf(__fsub_rn(Z, D10)) <= V.tau && fabsf(__fsub_rn(Z, D11)) <= V.tau;
        const bool cov = depth_valid(Dn, V.zn, V.zf) && !(e > V.tau) && !(-e > V.tau) && all_ok;
        if (!cov) continue;
        sum[29] += 1.0;
        if (INFO) {
            float qxf = X, qyf = Y, qzf = Z;
            if (framed) transform34(Fr, X, Y, Z, qxf, qyf, qzf);
            const double px = (double)qxf, py = (double)qyf, pz = (double)qzf;
            sum[0] += py * py + pz * pz;  sum[1] += -(px * py);         sum[2] += -(px * pz);
            sum[4] += -pz;                sum[5] += py;
            sum[6] += px * px + pz * pz;  sum[7] += -(py * pz);
            sum[8] += pz;                 sum[10] += -px;
            sum[11] += px * px + py * py;
            sum[12] += -py;               sum[13] += px;
            sum[15] += 1.0;               sum[18] += 1.0;               sum[20] += 1.0;
        } else {
            const double wx = (double)wxf, wy = (double)wyf, Xd = (double)X, Yd = (double)Y, Zd = (double)Z;
            const double iz = 1.0 / Zd;
            const double ux = fx * iz, uz = -((ux * Xd) * iz), vy = fy * iz, vz = -((vy * Yd) * iz);
            double J[6];
            {   // the photometric row, summed completely before the geometric one is formed
                const double c00 = (double)I00, c01 = (double)I01, c10 = (double)I10, c11 = (double)I11;
                const double top = c00 + wx * (c01 - c00), bot = c10 + wx * (c11 - c10);
                const double L = top + wy * (bot - top);
                const double Lu = (c01 - c00) + wy * ((c11 - c10) - (c01 - c00)), Lv = bot - top;
                row_of(sp, Xd, Yd, Zd, -(Lu * ux), -(Lv * vy), -(Lu * uz + Lv * vz), J);
                add_row(sum, J, sp * ((double)Is - L));
            }
            {
                const double c00 = (double)D00, c01 = (double)D01, c10 = (double)D10, c11 = (double)D11;
                const double top = c00 + wx * (c01 - c00), bot = c10 + wx * (c11 - c10);
                const double L = top + wy * (bot - top);
                const double Lu = (c01 - c00) + wy * ((c11 - c10) - (c01 - c00)), Lv = bot - top;
                const double ez = Zd - L;
                row_of(sg, Xd, Yd, Zd, -(Lu * ux), -(Lv * vy), 1.0 - (Lu * uz + Lv * vz), J);
                add_row(sum, J, sg * ez);
                sum[28] += ez * ez;
            }
        }
    }
    block_sum_f64<ODO_SLOTS>(sum, partial + (int64_t)p * gridDim.x * ODO_SLOTS);
}

__device__ __forceinline__ bool pivot_fails(double pivot, double ajj) { return !finite_f64(pivot) || pivot <= ODO_PIVOT_REL * ajj; }
__device__ __forceinline__ int tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }      // slot of (a, b), a <= b

// grid (P), 64 lanes: the fold of a pair's workgroup sums, then (row >= 0) the update rule of point_icp.hip's icp_update_kernel
__global__ __launch_bounds__(64) void rgbd_update_kernel(const double *__restrict__ partials, int blocks, int row_index, int rows,
                                                         int level_first, double rel_fitness, double rel_rmse, double *__restrict__ states,
                                                         double *__restrict__ history, double *__restrict__ sums) {
    __shared__ double sum[ODO_SLOTS];
    __shared__ double A[6][6], L[6][6], x[6];
    const int lane = threadIdx.x, p = blockIdx.x;
    double *__restrict__ state = states ? states + (int64_t)p * ODO_STATE : nullptr;
    const bool step = row_index >= 0;
    double status_in = step ? state[18] : 0.0;
    if (step && level_first != 0 && status_in == 1.0) status_in = 0.0;          // a coarser level's convergence does not bind this one
    const bool frozen = status_in != 0.0;
    if (!frozen && lane < ODO_SLOTS) {
        const double *__restrict__ src = partials + (int64_t)p * blocks * ODO_SLOTS + lane;
        double t = 0.0;
        for (int b = 0; b < blocks; ++b) t += src[(int64_t)b * ODO_SLOTS];
        sum[lane] = t;
        if (sums) sums[(int64_t)p * ODO_SLOTS + lane] = t;
    }
    __syncthreads();
    if (lane != 0 || !step) return;
    double *hrow = history + ((int64_t)p * rows + row_index) * ODO_ROW;
    if (frozen) {
        hrow[0] = state[16]; hrow[1] = state[17]; hrow[2] = state[20]; hrow[3] = state[21];
        hrow[4] = 0.0; hrow[5] = 0.0; hrow[6] = state[18]; hrow[7] = 0.0;
        return;
    }
    const double count = sum[29], fitness = count / sum[30], rmse = sqrt(sum[28] / count);
    const double prev_fitness = state[16], prev_rmse = state[17];
    double status = 0.0, wn = 0.0, vn = 0.0;
    if (count < 6.0) {
        status = 2.0;
    } else if (level_first == 0 && fabs(fitness - prev_fitness) < rel_fitness && fabs(rmse - prev_rmse) < rel_rmse) {
        status = 1.0;
    } else {
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { A[a][b] = sum[tri(a, b)]; A[b][a] = A[a][b]; }
        for (int j = 0; j < 6 && status == 0.0; ++j) {
            double piv = A[j][j];
            for (int k = 0; k < j; ++k) piv -= L[j][k] * L[j][k];
            if (pivot_fails(piv, A[j][j])) { status = 2.0; break; }
            const double d = sqrt(piv);
            L[j][j] = d;
            for (int i = j + 1; i < 6; ++i) {
                double t = A[i][j];
                for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
                L[i][j] = t / d;
            }
        }
    }
    if (status == 0.0) {
        for (int i = 0; i < 6; ++i) {                                         // L y = J^T r
            double t = sum[21 + i];
            for (int k = 0; k < i; ++k) t -= L[i][k] * x[k];
            x[i] = t / L[i][i];
        }
        for (int i = 5; i >= 0; --i) {                                        // L^T z = y
            double t = x[i];
            for (int k = i + 1; k < 6; ++k) t -= L[k][i] * x[k];
            x[i] = t / L[i][i];
        }
        const double wx = -x[0], wy = -x[1], wz = -x[2], vx = -x[3], vy = -x[4], vz = -x[5];
        const double th2 = (wx * wx + wy * wy) + wz * wz;
        double a = 1.0, b = 0.5;
        if (!(th2 < ODO_SMALL_THETA2)) {
            const double th = sqrt(th2);
            a = sin(th) / th;
            b = (1.0 - cos(th)) / th2;
        }
        wn = sqrt(th2);
        vn = sqrt((vx * vx + vy * vy) + vz * vz);
        const double R[9] = {1.0 + b * (wx * wx - th2), -(a * wz) + b * (wx * wy), a * wy + b * (wx * wz),
                             a * wz + b * (wx * wy), 1.0 + b * (wy * wy - th2), -(a * wx) + b * (wy * wz),
                             -(a * wy) + b * (wx * wz), a * wx + b * (wy * wz), 1.0 + b * (wz * wz - th2)};
        const double v[3] = {vx, vy, vz};
        double Tn[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double t = (R[r * 3] * state[c] + R[r * 3 + 1] * state[4 + c]) + R[r * 3 + 2] * state[8 + c];
                if (c == 3) t += v[r];
                Tn[r * 4 + c] = t;
            }
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) state[k] = Tn[k];
        state[19] += 1.0;
    }
    state[16] = fitness; state[17] = rmse; state[18] = status; state[20] = count; state[21] = sum[27];
    hrow[0] = fitness; hrow[1] = rmse; hrow[2] = count; hrow[3] = sum[27]; hrow[4] = wn; hrow[5] = vn; hrow[6] = status; hrow[7] = 0.0;
}

static bool sizes_ok(int32_t H, int32_t W, int32_t P) { return H >= 2 && W >= 2 && P >= 1 && P <= 65535 && (int64_t)H * W < (1ll << 31); }

}  // namespace

extern "C" int sgam_rgbd_pyramid_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t H, int32_t W, int32_t levels,
                                     float *intensity, float *depth, void *stream) {
    if (!depth_ptrs || !rgb_ptrs || !intensity || !depth || F < 1 || H < 2 || W < 2 || levels < 1 || levels > ODO_MAX_LEVELS ||
        (int64_t)F * H * W >= (1ll << 31))
        return SGAM_EINVAL;
    int h = H, w = W;
    for (int l = 1; l < levels; ++l) {                                        // a level smaller than 2 x 2 is refused
        h = (h + 1) / 2; w = (w + 1) / 2;
        if (h < 2 || w < 2) return SGAM_EINVAL;
    }
    hipStream_t s = sgam_stream(stream);
    int64_t n = (int64_t)F * H * W;
    SGAM_KLAUNCH(rgbd_pyramid_base_kernel, dim3(blocks_of(n)), dim3(256), 0, s, (const float *const *)depth_ptrs,
                 (const uint8_t *const *)rgb_ptrs, (int64_t)H * W, n, intensity, depth);
    h = H; w = W;
    int64_t off = 0;
    for (int l = 1; l < levels; ++l) {
        const int ho = (h + 1) / 2, wo = (w + 1) / 2;
        const int64_t no = (int64_t)F * ho * wo;
        SGAM_KLAUNCH(rgbd_pyramid_down_kernel, dim3(blocks_of(no)), dim3(256), 0, s, (const float *)(intensity + off),
                     (const float *)(depth + off), h, w, ho, wo, no, intensity + off + n, depth + off + n);
        off += n; n = no; h = ho; w = wo;
    }
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_rgbd_odometry_workspace_bytes(int32_t H, int32_t W, int32_t P) {
    if (!sizes_ok(H, W, P)) return SGAM_EINVAL;
    return r16((int64_t)P * chunks_of((int64_t)H * W) * ODO_SLOTS * 8);       // the per-workgroup sums
}

extern "C" int sgam_rgbd_odometry_accumulate_f32(const void *depth_ptrs, const void *intensity_ptrs, int32_t F, int32_t H, int32_t W,
                                                 const float *kinv9, float fx, float fy, float cx, float cy, float z_near, float z_far,
                                                 float max_depth_diff, double lambda_geometric, const int32_t *pairs, const double *state,
                                                 int32_t P, int32_t level_first, int32_t information, const float *frames, void *workspace,
                                                 int64_t workspace_bytes, void *stream) {
    if (!depth_ptrs || !intensity_ptrs || !kinv9 || !pairs || !state || F < 1 || !(max_depth_diff >= 0.0f) || !(z_near <= z_far) ||
        !(lambda_geometric >= 0.0 && lambda_geometric <= 1.0) || (frames && !information))
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_rgbd_odometry_workspace_bytes(H, W, P))) return SGAM_EINVAL;
    OdoView V;
    for (int i = 0; i < 9; ++i) V.kinv[i] = kinv9[i];
    V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy; V.zn = z_near; V.zf = z_far; V.tau = max_depth_diff;
    V.H = H; V.W = W; V.F = F;
    const dim3 grid((unsigned)chunks_of((int64_t)H * W), (unsigned)P);
    hipStream_t s = sgam_stream(stream);
    if (information)
        SGAM_KLAUNCH(rgbd_accumulate_kernel<true>, grid, dim3(256), 0, s, V, (const float *const *)depth_ptrs,
                     (const float *const *)intensity_ptrs, pairs, state, frames, lambda_geometric, 0, (double *)workspace);
    else
        SGAM_KLAUNCH(rgbd_accumulate_kernel<false>, grid, dim3(256), 0, s, V, (const float *const *)depth_ptrs,
                     (const float *const *)intensity_ptrs, pairs, state, frames, lambda_geometric, level_first != 0 ? 1 : 0,
                     (double *)workspace);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_rgbd_odometry_update(const void *workspace, int64_t workspace_bytes, int32_t H, int32_t W, int32_t P, int32_t row,
                                         int32_t rows, int32_t level_first, double relative_fitness, double relative_rmse, double *state,
                                         double *history, double *sums, void *stream) {
    const bool step = row >= 0;
    if (step ? (!state || !history || row >= rows || !(relative_fitness >= 0.0) || !(relative_rmse >= 0.0)) : (!sums || row != -1))
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_rgbd_odometry_workspace_bytes(H, W, P))) return SGAM_EINVAL;
    SGAM_KLAUNCH(rgbd_update_kernel, dim3((unsigned)P), dim3(64), 0, sgam_stream(stream), (const double *)workspace,
                 (int)chunks_of((int64_t)H * W), (int)row, (int)rows, level_first != 0 ? 1 : 0, relative_fitness, relative_rmse, state, history,
                 sums);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
