// point_cells.h — what a search over a uniform grid of POINTS is made of, shared by point_nn.hip (nearest neighbours) and
// point_segment.hip (fixed-radius walks): the cells' records and the sink that keeps the nearest candidate, written ONCE.  The
// grid, its build and the shell walk are grid_common.h's; point_nn.hip's header has the stop rule and its proof.
#pragma once
#include "grid_common.h"

namespace {

constexpr int POINT_RECORD = 16;              // bytes of a record of the grid's cell-sorted table: (x, y, z, id)

struct NearestSink {
    float best = __uint_as_float(0x7f800000u);
    int bi = -1;
    __device__ __forceinline__ void offer(float d2, int id, float max_d2) {
        const bool take = (d2 <= max_d2) & ((d2 < best) | ((d2 == best) & (id < bi)));        // (+inf == +inf: id < -1 never holds)
        best = take ? d2 : best;                                              // (selects, no branch: one compare chain per pair)
        bi = take ? id : bi;
    }
    __device__ __forceinline__ float bound() const { return best; }
};

// a cell's records are (x, y, z, id); the stop rule's factor 1 - 2^-18 (point_nn.hip's header)
struct PointCells {
    const float4 *__restrict__ sorted;
    static __device__ __forceinline__ float shrink() { return 0.99999618530273437500f; }
    template <class Sink>
    __device__ __forceinline__ void scan(int s, int e, float qx, float qy, float qz, float max_d2, Sink &sink) const {
        for (int k = s; k < e; ++k) {
            const float4 p = sorted[k];
            sink.offer(dist2(p.x, p.y, p.z, qx, qy, qz), __float_as_int(p.w), max_d2);
        }
    }
};

}  // namespace
