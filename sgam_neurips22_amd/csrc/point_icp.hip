// point_icp.hip — rigid registration (ICP) of one cloud onto another on top of the nearest-neighbour search of point_nn.hip: the
// source moved by the current pose (sgam_points_transform_f32), the normal equations of one Gauss-Newton step summed over the
// correspondences (sgam_points_icp_accumulate) and the step itself with its stop rules (sgam_points_icp_update).  The pose, the
// stop state and the history live on the device: an iteration is four launches (transform, search, accumulate, update) and reads
// nothing back.  "not a point", transform34 and the fold of a chunk sum are points_common.h's; tests/icp_oracle.py restates the
// rules in numpy.  No float atomics; every output is a function of the inputs only.  DESIGN §4.4.6.
//
// Transform: T = 16 DEVICE doubles, a row-major 4 x 4.  T[0..11] are rounded to fp32 once and applied with transform34, the
// unprojection's expression; a point that is not a point comes out NaN.
//
// Accumulate: one workgroup per chunk of ICP_CHUNK = 4096 source points, a lane takes the points base + c * 256 + lane in ascending
// c.  Entry i is a CORRESPONDENCE iff 0 <= index[i] (< Nr: an index past the target is refused rather than read) and, with normals,
// finite3(normal[index[i]]).  Per correspondence, in fp64 on the widened fp32 inputs, p = moved[i], q = target[index[i]],
// n = normal[index[i]], e = (p.x - q.x, p.y - q.y, p.z - q.z); the summand of every slot, one IEEE operation per operator:
//   point-to-plane (normals given):   c = (p.y n.z - p.z n.y,  p.z n.x - p.x n.z,  p.x n.y - p.y n.x),  J = (c.x, c.y, c.z, n.x, n.y, n.z)
//                                     r = (e.x n.x + e.y n.y) + e.z n.z
//       slot of (a, b), a <= b: J[a] * J[b]        slot 21 + a: J[a] * r        slot 27: r * r
//   point-to-point (normals NULL), the three rows J = [-[p]x | I] with residuals e, the products summed per point:
//       rows 0..2 x columns 0..2:  (0,0) p.y p.y + p.z p.z   (0,1) -(p.x p.y)   (0,2) -(p.x p.z)
//                                  (1,1) p.x p.x + p.z p.z   (1,2) -(p.y p.z)   (2,2) p.x p.x + p.y p.y
//       rows 0..2 x columns 3..5:  (0,3) 0  (0,4) -p.z  (0,5) p.y     (1,3) p.z  (1,4) 0  (1,5) -p.x     (2,3) -p.y  (2,4) p.x  (2,5) 0
//       rows 3..5 x columns 3..5:  1 on the diagonal, 0 off it
//       slots 21..23: p.y e.z - p.z e.y,  p.z e.x - p.x e.z,  p.x e.y - p.y e.x        slots 24..26: e.x, e.y, e.z
//       slot 27: (e.x e.x + e.y e.y) + e.z e.z
//   both: slot 28: (double)d2[i]    slot 29: 1    slot 30: 1 for every source point of the chunk with finite3(moved[i]), a
//   correspondence or not    slot 31: 0.
// The upper triangle is stored row-major: (0,0..5) = slots 0..5, (1,1..5) = 6..10, (2,2..5) = 11..14, (3,3..5) = 15..17,
// (4,4..5) = 18..19, (5,5) = 20.  Each slot is summed per lane in index order and folded by block_sum_f64.
//
// Update: one wavefront.  Lane s < 32 folds slot s over the chunks in ascending order; lane 0 does everything after that, in fp64:
//   state[0..15] T, [16] previous fitness, [17] previous RMSE, [18] status (0 running, 1 converged, 2 degenerate), [19] iterations
//   applied, [20] correspondences and [21] sum r^2 of the last evaluated iteration, [22..23] 0.
//   history row `iteration` = {fitness, RMSE, correspondences, sum r^2, |omega|, |v|, status after this call, 0}.
//   1. status != 0: the row is {state[16], state[17], state[20], state[21], 0, 0, status, 0} and nothing else changes.
//   2. fitness = count / points, rmse = sqrt(sum d2 / count) (Open3D's definition: point distances whatever the estimation);
//      these four go to state[16], [17], [20], [21] in every branch below.
//   3. count < 6: status 2, T untouched.
//   4. iteration > 0 and |fitness - previous| < relative_fitness and |rmse - previous| < relative_rmse: status 1, T untouched.
//   5. A = L L^T by Cholesky, column by column; the pivot of column j is A_jj - sum_k<j L_jk^2; not finite or <= ICP_PIVOT_REL * A_jj:
//      status 2, T untouched.
//   6. xi = -(A^-1 J^T r) by the two triangular solves, omega = xi[0..2], v = xi[3..5]; theta^2 = omega . omega;
//      a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2, or 1 and 1/2 when theta^2 < 1e-16;
//      dR = I + a [omega]x + b (omega omega^T - theta^2 I);  T <- [dR | v] T;  iterations += 1.
//
// Coloured ICP (Park, Zhou, Koltun, ICCV 2017; Open3D's registration_colored_icp as documented): where the geometry leaves the pose
// free (a plane) the colours of the two clouds pin it.  Intensity of a point with the uint8 colour (r, g, b):
// I = (double)(r + g + b) / 765.0, the sum an integer.  tests/colored_icp_oracle.py restates both kernels.
//
// Colour gradient (sgam_points_color_gradient_f32): one lane per point p with normal n, over the entries 0 <= j < N of its k-NN row
// (the point itself excluded by the search) in ascending column order, in fp64 on the widened inputs:
//   e = p_j - p;  en = (e.x n.x + e.y n.y) + e.z n.z;  u = e - en * n (per component);  A_ab += u_a * u_b (upper triangle);
//   b_a += u_a * (I_j - I_p);  m += 1.
// Then the tangent-plane constraint, Open3D's extra row m * n with right-hand side 0:  A_ab += (double)(m * m) * (n_a * n_b).
// A g = b by a 3 x 3 Cholesky in the update's order and with its pivot rule (a pivot A_jj - sum_k<j L_jk^2 that is not finite or
// <= ICP_PIVOT_REL * A_jj fails), then the two triangular solves.  NaN x 3 for a p that is not a point, an n that is not finite,
// m < 3 or a failed factorisation; otherwise g rounded to fp32 once.
//
// Coloured accumulate (sgam_points_icp_accumulate_colored): the chunking, the fold and the 32 slots of the accumulation above, so
// that the update is used unchanged.  Entry i is a correspondence iff 0 <= index[i] < Nr and the normal AND the gradient at
// index[i] are finite.  With p = moved[i], q, n, d = the target's point, normal, gradient, I_s / I_t the two intensities,
// e = p - q, sg = sqrt(lambda), sp = sqrt(1 - lambda), en = (e.x n.x + e.y n.y) + e.z n.z:
//   geometric row:    c = p x n (point-to-plane's expressions),  J_G = (sg c.x, sg c.y, sg c.z, sg n.x, sg n.y, sg n.z),  r_G = sg * en
//   photometric row:  w = e - en * n;  I_proj = ((d.x w.x + d.y w.y) + d.z w.z) + I_t;  dn = (d.x n.x + d.y n.y) + d.z n.z;
//                     dM = -d + dn * n;  c = p x dM (the same expressions, dM for n);  J_I = sp * (c, dM);  r_I = sp * (I_s - I_proj)
//   slots 0..20 += J_G[a] * J_G[b], then += J_I[a] * J_I[b];  21..26 += J_G[a] * r_G, then += J_I[a] * r_I;  27 += r_G * r_G, then
//   += r_I * r_I;  28..31 as above.  lambda = 1: sg = 1, sp = 0, the point-to-plane sums bit for bit.
#include "points_common.h"

#include <cmath>

namespace {

constexpr int ICP_CHUNK = 4096;               // source points per workgroup of the accumulation (256 lanes x 16)
constexpr int ICP_SLOTS = 32;
// A Cholesky pivot at or below this share of the matrix's own diagonal entry means that the correspondences leave a direction of
// the pose free (a plane slides along itself): the step would be huge and meaningless.  Not a tuned number: fp64 leaves 1e-16.
constexpr double ICP_PIVOT_REL = 1e-12;
constexpr double ICP_SMALL_THETA2 = 1e-16;

__global__ __launch_bounds__(256) void transform_kernel(const float *__restrict__ points, int N, const double *__restrict__ T64,
                                                        float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = (float)T64[k];
    const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
    const float nanf_ = __uint_as_float(0x7fc00000u);
    float X = nanf_, Y = nanf_, Z = nanf_;
    if (finite3(x, y, z)) transform34(T, x, y, z, X, Y, Z);
    out[i * 3] = X; out[i * 3 + 1] = Y; out[i * 3 + 2] = Z;
}

__device__ __forceinline__ double intensity(const uint8_t *__restrict__ colors, int64_t i) {
    return (double)((int)colors[i * 3] + (int)colors[i * 3 + 1] + (int)colors[i * 3 + 2]) / 765.0;
}

// the pivot rule of both Cholesky factorisations: the pivot of column j against the matrix's own A_jj
__device__ __forceinline__ bool pivot_fails(double pivot, double ajj) { return !finite_f64(pivot) || pivot <= ICP_PIVOT_REL * ajj; }

// one row of the normal equations into the slots: J[a] * J[b], J[a] * r, r * r
__device__ __forceinline__ void add_row(double (&s)[ICP_SLOTS], double j0, double j1, double j2, double j3, double j4, double j5, double r) {
    const double J[6] = {j0, j1, j2, j3, j4, j5};
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

enum { ICP_POINT = 0, ICP_PLANE = 1, ICP_COLORED = 2 };

// the chunk skeleton of the three estimations; source_colors, target_colors, gradient and lambda are read by ICP_COLORED only,
// normals by all but ICP_POINT
template <int EST>
__global__ __launch_bounds__(256) void icp_accumulate_kernel(const float *__restrict__ moved, const uint8_t *__restrict__ source_colors,
                                                             const float *__restrict__ target, const float *__restrict__ normals,
                                                             const uint8_t *__restrict__ target_colors, const float *__restrict__ gradient,
                                                             const int32_t *__restrict__ index, const float *__restrict__ d2, int N, int Nr,
                                                             double lambda, double *__restrict__ partial) {
    const int64_t base = (int64_t)blockIdx.x * ICP_CHUNK;
    const double sg = sqrt(lambda), sp = sqrt(1.0 - lambda);
    double s[ICP_SLOTS];
#pragma unroll
    for (int k = 0; k < ICP_SLOTS; ++k) s[k] = 0.0;
    for (int c = 0; c < ICP_CHUNK / 256; ++c) {
        const int64_t i = base + c * 256 + threadIdx.x;
        if (i >= N) break;
        const float fx = moved[i * 3], fy = moved[i * 3 + 1], fz = moved[i * 3 + 2];
        if (finite3(fx, fy, fz)) s[30] += 1.0;
        const int j = index[i];
        if (j < 0 || j >= Nr) continue;
        float hx = 0.0f, hy = 0.0f, hz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f;
        if (EST != ICP_POINT) {
            hx = normals[(int64_t)j * 3]; hy = normals[(int64_t)j * 3 + 1]; hz = normals[(int64_t)j * 3 + 2];
            if (!finite3(hx, hy, hz)) continue;
        }
        if (EST == ICP_COLORED) {
            tx = gradient[(int64_t)j * 3]; ty = gradient[(int64_t)j * 3 + 1]; tz = gradient[(int64_t)j * 3 + 2];
            if (!finite3(tx, ty, tz)) continue;
        }
        const double px = (double)fx, py = (double)fy, pz = (double)fz;
        const double ex = px - (double)target[(int64_t)j * 3], ey = py - (double)target[(int64_t)j * 3 + 1],
                     ez = pz - (double)target[(int64_t)j * 3 + 2];
        if (EST == ICP_POINT) {
            s[0] += py * py + pz * pz;  s[1] += -(px * py);         s[2] += -(px * pz);
            s[4] += -pz;                s[5] += py;
            s[6] += px * px + pz * pz;  s[7] += -(py * pz);
            s[8] += pz;                 s[10] += -px;
            s[11] += px * px + py * py;
            s[12] += -py;               s[13] += px;
            s[15] += 1.0;               s[18] += 1.0;               s[20] += 1.0;
            s[21] += py * ez - pz * ey; s[22] += pz * ex - px * ez; s[23] += px * ey - py * ex;
            s[24] += ex;                s[25] += ey;                s[26] += ez;
            s[27] += (ex * ex + ey * ey) + ez * ez;
        } else {
            const double nx = (double)hx, ny = (double)hy, nz = (double)hz;
            const double en = (ex * nx + ey * ny) + ez * nz;
            if (EST == ICP_PLANE) {
                add_row(s, py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz, en);
            } else {
                // the geometric row, summed completely before the photometric one is formed: one row's products live at a time
                add_row(s, sg * (py * nz - pz * ny), sg * (pz * nx - px * nz), sg * (px * ny - py * nx), sg * nx, sg * ny, sg * nz, sg * en);
                const double dx = (double)tx, dy = (double)ty, dz = (double)tz;
                const double wx = ex - en * nx, wy = ey - en * ny, wz = ez - en * nz;
                const double Iproj = ((dx * wx + dy * wy) + dz * wz) + intensity(target_colors, j);
                const double dn = (dx * nx + dy * ny) + dz * nz;
                const double mx = -dx + dn * nx, my = -dy + dn * ny, mz = -dz + dn * nz;
                add_row(s, sp * (py * mz - pz * my), sp * (pz * mx - px * mz), sp * (px * my - py * mx), sp * mx, sp * my, sp * mz,
                        sp * (intensity(source_colors, i) - Iproj));
            }
        }
        s[28] += (double)d2[i];
        s[29] += 1.0;
    }
    block_sum_f64(s, partial);
}

// one lane per point; the loop over the row stays rolled and nothing is indexed by anything but c: no private memory
__global__ __launch_bounds__(256) void color_gradient_kernel(const float *__restrict__ points, const float *__restrict__ normals,
                                                             const uint8_t *__restrict__ colors, int N, const int32_t *__restrict__ knn_index,
                                                             int k, float *__restrict__ gradient) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float fx = points[i * 3], fy = points[i * 3 + 1], fz = points[i * 3 + 2];
    const float hx = normals[i * 3], hy = normals[i * 3 + 1], hz = normals[i * 3 + 2];
    const float nanf_ = __uint_as_float(0x7fc00000u);
    float gx = nanf_, gy = nanf_, gz = nanf_;
    if (finite3(fx, fy, fz) && finite3(hx, hy, hz)) {
        const double px = (double)fx, py = (double)fy, pz = (double)fz, nx = (double)hx, ny = (double)hy, nz = (double)hz;
        const double Ip = intensity(colors, i);
        double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
        int m = 0;
#pragma unroll 1
        for (int c = 0; c < k; ++c) {
            const int j = knn_index[i * k + c];
            if (j < 0 || j >= N) continue;
            const double ex = (double)points[(int64_t)j * 3] - px, ey = (double)points[(int64_t)j * 3 + 1] - py,
                         ez = (double)points[(int64_t)j * 3 + 2] - pz;
            const double en = (ex * nx + ey * ny) + ez * nz;
            const double ux = ex - en * nx, uy = ey - en * ny, uz = ez - en * nz;
            const double dI = intensity(colors, j) - Ip;
            axx += ux * ux; axy += ux * uy; axz += ux * uz; ayy += uy * uy; ayz += uy * uz; azz += uz * uz;
            bx += ux * dI; by += uy * dI; bz += uz * dI;
            ++m;
        }
        if (m >= 3) {
            const double mm = (double)(m * m);
            axx += mm * (nx * nx); axy += mm * (nx * ny); axz += mm * (nx * nz);
            ayy += mm * (ny * ny); ayz += mm * (ny * nz); azz += mm * (nz * nz);
            // A = L L^T column by column, then L y = b and L^T g = y: the update's order and pivot rule
            const double p0 = axx;
            if (!pivot_fails(p0, axx)) {
                const double l00 = sqrt(p0), l10 = axy / l00, l20 = axz / l00;
                const double p1 = ayy - l10 * l10;
                if (!pivot_fails(p1, ayy)) {
                    const double l11 = sqrt(p1), l21 = (ayz - l20 * l10) / l11;
                    const double p2 = (azz - l20 * l20) - l21 * l21;
                    if (!pivot_fails(p2, azz)) {
                        const double l22 = sqrt(p2);
                        const double y0 = bx / l00, y1 = (by - l10 * y0) / l11, y2 = ((bz - l20 * y0) - l21 * y1) / l22;
                        const double g2 = y2 / l22, g1 = (y1 - l21 * g2) / l11, g0 = ((y0 - l10 * g1) - l20 * g2) / l00;
                        gx = (float)g0; gy = (float)g1; gz = (float)g2;
                    }
                }
            }
        }
    }
    gradient[i * 3] = gx; gradient[i * 3 + 1] = gy; gradient[i * 3 + 2] = gz;
}

__device__ __forceinline__ int tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }      // slot of (a, b), a <= b

__global__ __launch_bounds__(64) void icp_update_kernel(const double *__restrict__ partials, int blocks, int iteration, double rel_fitness,
                                                        double rel_rmse, double *__restrict__ state, double *__restrict__ history) {
    __shared__ double sum[ICP_SLOTS];
    __shared__ double A[6][6], L[6][6], x[6];
    const int lane = threadIdx.x;
    const bool frozen = state[18] != 0.0;
    if (!frozen && lane < ICP_SLOTS) {
        double t = 0.0;
        for (int b = 0; b < blocks; ++b) t += partials[(int64_t)b * ICP_SLOTS + lane];
        sum[lane] = t;
    }
    __syncthreads();
    if (lane != 0) return;
    double *row = history + (int64_t)iteration * 8;
    if (frozen) {
        row[0] = state[16]; row[1] = state[17]; row[2] = state[20]; row[3] = state[21];
        row[4] = 0.0; row[5] = 0.0; row[6] = state[18]; row[7] = 0.0;
        return;
    }
    const double count = sum[29], fitness = count / sum[30], rmse = sqrt(sum[28] / count);
    const double prev_fitness = state[16], prev_rmse = state[17];
    double status = 0.0, wn = 0.0, vn = 0.0;
    if (count < 6.0) {
        status = 2.0;
    } else if (iteration > 0 && fabs(fitness - prev_fitness) < rel_fitness && fabs(rmse - prev_rmse) < rel_rmse) {
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
        if (!(th2 < ICP_SMALL_THETA2)) {
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
    row[0] = fitness; row[1] = rmse; row[2] = count; row[3] = sum[27]; row[4] = wn; row[5] = vn; row[6] = status; row[7] = 0.0;
}

}  // namespace

extern "C" int sgam_points_transform_f32(const float *points, int32_t N, const double *T, float *out, void *stream) {
    if (!points || !T || !out || N < 1) return SGAM_EINVAL;
    SGAM_KLAUNCH(transform_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), points, N, T, out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_points_icp_partials(int64_t n) {
    if (n < 1) return SGAM_EINVAL;
    return ICP_SLOTS * ((n + ICP_CHUNK - 1) / ICP_CHUNK);
}

template <int EST>
static int launch_accumulate(const float *moved, const uint8_t *source_colors, const float *target, const float *normals,
                             const uint8_t *target_colors, const float *gradient, const int32_t *index, const float *d2, int32_t N, int32_t Nr,
                             double lambda, double *partials, void *stream) {
    const dim3 grid((unsigned)(((int64_t)N + ICP_CHUNK - 1) / ICP_CHUNK));
    SGAM_KLAUNCH(icp_accumulate_kernel<EST>, grid, dim3(256), 0, sgam_stream(stream), moved, source_colors, target, normals, target_colors,
                 gradient, index, d2, N, Nr, lambda, partials);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_icp_accumulate(const float *moved, const float *target, const float *target_normals, const int32_t *index,
                                          const float *d2, int32_t N, int32_t Nr, double *partials, void *stream) {
    if (!moved || !target || !index || !d2 || !partials || N < 1 || Nr < 1) return SGAM_EINVAL;
    const auto launch = target_normals ? launch_accumulate<ICP_PLANE> : launch_accumulate<ICP_POINT>;
    return launch(moved, nullptr, target, target_normals, nullptr, nullptr, index, d2, N, Nr, 1.0, partials, stream);
}

extern "C" int sgam_points_color_gradient_f32(const float *points, const float *normals, const uint8_t *colors, int32_t N,
                                              const int32_t *knn_index, int32_t k, float *gradient_out, void *stream) {
    if (!points || !normals || !colors || !knn_index || !gradient_out || N < 1 || k < 1 || k > KNN_MAX_K) return SGAM_EINVAL;
    SGAM_KLAUNCH(color_gradient_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), points, normals, colors, N, knn_index, k,
                 gradient_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_icp_accumulate_colored(const float *moved, const uint8_t *source_colors, const float *target,
                                                  const float *target_normals, const uint8_t *target_colors, const float *target_gradient,
                                                  const int32_t *index, const float *d2, int32_t N, int32_t Nr, double lambda_geometric,
                                                  double *partials, void *stream) {
    if (!moved || !source_colors || !target || !target_normals || !target_colors || !target_gradient || !index || !d2 || !partials || N < 1 ||
        Nr < 1 || !(lambda_geometric >= 0.0 && lambda_geometric <= 1.0))
        return SGAM_EINVAL;
    return launch_accumulate<ICP_COLORED>(moved, source_colors, target, target_normals, target_colors, target_gradient, index, d2, N, Nr,
                                          lambda_geometric, partials, stream);
}

extern "C" int sgam_points_icp_update(const double *partials, int64_t blocks, int32_t iteration, double relative_fitness, double relative_rmse,
                                      double *state, double *history, void *stream) {
    if (!partials || !state || !history || blocks < 1 || blocks > 0x7fffffffll / ICP_SLOTS || iteration < 0 || !(relative_fitness >= 0.0) ||
        !(relative_rmse >= 0.0))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(icp_update_kernel, dim3(1), dim3(64), 0, sgam_stream(stream), partials, (int)blocks, (int)iteration, relative_fitness,
                 relative_rmse, state, history);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
