/* mppi_peers_math.inc -- the arithmetic gpd_mppi_peers (include/gpd.h) adds to the planner's cost: the hinge on the distance to ONE
 * peer, and the running minimum of those distances.  fp32 throughout.  Plain C, like mppi_math.inc: the kernel in mppi_peers.inc and the
 * host program tests/c/mppi_peers_host.c compile THIS text.  The reference has no such code: it has no planner.  Included after gpd.h. */
#ifndef GPD_MPPI_PEERS_MATH_INC
#define GPD_MPPI_PEERS_MATH_INC

#ifndef GPD_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_HOST_DEVICE __host__ __device__
#else
#include <math.h>
#define GPD_HOST_DEVICE
#pragma clang fp contract(off)      /* as the device build (-ffp-contract=off) */
#endif
#endif

#ifndef GPD_OBST_INF
#define GPD_OBST_INF (__builtin_inff())
#endif

/* the distance to a peer at the offset (dx, dy, dz); NaN for an offset that is not finite in a way that does not cancel (a NaN row;
 * +inf for an infinite one) */
GPD_HOST_DEVICE static inline float gpd_mppi_peer_distance(float dx, float dy, float dz) { return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))); }

/* the hinge of one peer: max(0, peer_dist - d)^2.  d = 0 (the peer at the drone's own point) gives peer_dist^2; a row that is not
 * finite gives 0 (fmaxf drops the NaN, +inf is beyond every peer_dist).  Continuous and C1 in the offset: at d = peer_dist value and
 * slope are both 0, so nothing in it can flip between fp32 and fp64 */
GPD_HOST_DEVICE static inline float gpd_mppi_peer_pen(float peer_dist, float dx, float dy, float dz) {
    const float pen = fmaxf(0.0f, peer_dist - gpd_mppi_peer_distance(dx, dy, dz));
    return pen * pen;
}

/* the nearest peer so far: starts at GPD_OBST_INF; the comparison is false for a NaN, which is then not counted */
GPD_HOST_DEVICE static inline float gpd_mppi_peer_nearest(float d, float best) { return d < best ? d : best; }

#endif
