/* obstacle_math.inc -- the geometry of gpd_obstacles (include/gpd.h): for each kind of obstacle the exact signed distance from a
 * point with its unit gradient, and the first entry of a ray.  An obstacle is GPD_OBST_FLOATS floats  cx, cy, cz, kind, ax, ay,
 * az, 0; the functions take the point (or the ray's origin) RELATIVE to the centre, v = p - c.  fp32 throughout.
 * Plain C, on purpose: the kernels in obstacles.inc and the host program tests/c/obstacle_host.c compile THIS text, so the formulas a
 * machine without a GPU holds against the float64 restatement (tests/helpers/obstacles_f64.py) are the ones the device runs.  The
 * reference has no such code: its obstacles are Bullet bodies.  Included after gpd.h. */
#ifndef GPD_OBSTACLE_MATH_INC
#define GPD_OBSTACLE_MATH_INC

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_HOST_DEVICE __host__ __device__
#else
#include <math.h>
#define GPD_HOST_DEVICE
#pragma clang fp contract(off)      /* as the device build (-ffp-contract=off): the host rounds what the kernels round */
#endif

#define GPD_OBST_INF (__builtin_inff())

/* +1 for v >= 0 (and -0), -1 below: the side of a face a point on the centre plane is given to */
GPD_HOST_DEVICE static inline float gpd_obst_side(float v) { return v < 0.0f ? -1.0f : 1.0f; }

/* ---- (a) signed distance d (negative inside) and unit gradient n ------------------------------------------------------------ */

/* sphere of radius r; at the centre the gradient is (0, 0, 1) */
GPD_HOST_DEVICE static inline float gpd_sdf_sphere(float vx, float vy, float vz, float r, float* nx, float* ny, float* nz) {
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    const int at_centre = !(len > 0.0f);
    const float inv = 1.0f / (at_centre ? 1.0f : len);
    *nx = at_centre ? 0.0f : vx * inv;
    *ny = at_centre ? 0.0f : vy * inv;
    *nz = at_centre ? 1.0f : vz * inv;
    return len - r;
}

/* axis-aligned box of half extents (ax, ay, az): |max(q, 0)| + min(max(q), 0) with q = |v| - a.  Outside, the gradient points from
 * the nearest point of the surface; inside (and on the surface) it is the axis of least penetration, ties to the lower axis */
GPD_HOST_DEVICE static inline float gpd_sdf_box(float vx, float vy, float vz, float ax, float ay, float az, float* nx, float* ny, float* nz) {
    const float qx = fabsf(vx) - ax, qy = fabsf(vy) - ay, qz = fabsf(vz) - az;
    const float ox = fmaxf(qx, 0.0f), oy = fmaxf(qy, 0.0f), oz = fmaxf(qz, 0.0f);
    const float out = sqrtf(ox * ox + oy * oy + oz * oz);
    const float deepest = fmaxf(qx, fmaxf(qy, qz));
    const int outside = out > 0.0f;
    const float inv = 1.0f / (outside ? out : 1.0f);
    const int axis = (qx >= qy && qx >= qz) ? 0 : (qy >= qz ? 1 : 2);
    *nx = gpd_obst_side(vx) * (outside ? ox * inv : (axis == 0 ? 1.0f : 0.0f));
    *ny = gpd_obst_side(vy) * (outside ? oy * inv : (axis == 1 ? 1.0f : 0.0f));
    *nz = gpd_obst_side(vz) * (outside ? oz * inv : (axis == 2 ? 1.0f : 0.0f));
    return out + fminf(deepest, 0.0f);
}

/* vertical cylinder of radius r and half height h: the same form on q = (rho - r, |vz| - h), rho the distance from the axis.  On the
 * axis the radial direction is (1, 0, 0).  Inside, the side wins a tie against the cap */
GPD_HOST_DEVICE static inline float gpd_sdf_cylinder(float vx, float vy, float vz, float r, float h, float* nx, float* ny, float* nz) {
    const float rho = sqrtf(vx * vx + vy * vy);
    const int on_axis = !(rho > 0.0f);
    const float irho = 1.0f / (on_axis ? 1.0f : rho);
    const float ux = on_axis ? 1.0f : vx * irho, uy = on_axis ? 0.0f : vy * irho;
    const float qr = rho - r, qz = fabsf(vz) - h;
    const float orr = fmaxf(qr, 0.0f), oz = fmaxf(qz, 0.0f);
    const float out = sqrtf(orr * orr + oz * oz);
    const int outside = out > 0.0f;
    const float inv = 1.0f / (outside ? out : 1.0f);
    const float wr = outside ? orr * inv : (qr >= qz ? 1.0f : 0.0f);
    const float wz = outside ? oz * inv : (qr >= qz ? 0.0f : 1.0f);
    *nx = ux * wr;
    *ny = uy * wr;
    *nz = gpd_obst_side(vz) * wz;
    return out + fminf(fmaxf(qr, qz), 0.0f);
}

/* Any kind: the signed distance of the point v = p - c from the record (kind, ax, ay, az); GPD_OBST_NONE and unknown kinds are
 * infinitely far away (and never the nearest) */
GPD_HOST_DEVICE static inline float gpd_obst_sdf(int kind, float ax, float ay, float az, float vx, float vy, float vz, float* nx, float* ny,
                                                 float* nz) {
    switch (kind) {
    case GPD_OBST_SPHERE: return gpd_sdf_sphere(vx, vy, vz, ax, nx, ny, nz);
    case GPD_OBST_BOX: return gpd_sdf_box(vx, vy, vz, ax, ay, az, nx, ny, nz);
    case GPD_OBST_CYLINDER: return gpd_sdf_cylinder(vx, vy, vz, ax, az, nx, ny, nz);
    case GPD_OBST_FLOOR: *nx = 0.0f; *ny = 0.0f; *nz = 1.0f; return vz;
    default: *nx = 0.0f; *ny = 0.0f; *nz = 0.0f; return GPD_OBST_INF;
    }
}

/* ---- (b) first entry t >= 0 of the ray v + t d, |d| = 1: 0 for an origin inside or on the obstacle, +inf for a miss --------- */

/* the interval of t in which one coordinate v + t d lies in [-a, a], intersected into [*t0, *t1]; a direction parallel to the slab
 * (d == 0) decides by the origin alone and divides by nothing */
GPD_HOST_DEVICE static inline void gpd_ray_slab(float v, float d, float a, float* t0, float* t1) {
    if (d == 0.0f) {
        if (fabsf(v) > a) *t1 = -GPD_OBST_INF;
    } else {
        const float inv = 1.0f / d;
        const float ta = (-a - v) * inv, tb = (a - v) * inv;
        *t0 = fmaxf(*t0, fminf(ta, tb));
        *t1 = fminf(*t1, fmaxf(ta, tb));
    }
}

/* sphere: with b = v.d and c = |v|^2 - r^2 the entry is -b - sqrt(b^2 - c); evaluated without cancellation as c / (-b + sqrt(.)),
 * the discriminant from the ray's closest approach to the centre, r^2 - |v - b d|^2 */
GPD_HOST_DEVICE static inline float gpd_ray_sphere(float vx, float vy, float vz, float dx, float dy, float dz, float r) {
    const float b = vx * dx + vy * dy + vz * dz;
    const float c = (vx * vx + vy * vy + vz * vz) - r * r;
    const float px = vx - b * dx, py = vy - b * dy, pz = vz - b * dz;
    const float disc = r * r - (px * px + py * py + pz * pz);
    if (!(c > 0.0f)) return 0.0f;                       /* inside or on it */
    if (!(b < 0.0f) || !(disc >= 0.0f)) return GPD_OBST_INF;   /* points away, or passes by */
    return c / (sqrtf(disc) - b);
}

GPD_HOST_DEVICE static inline float gpd_ray_box(float vx, float vy, float vz, float dx, float dy, float dz, float ax, float ay, float az) {
    float t0 = 0.0f, t1 = GPD_OBST_INF;
    gpd_ray_slab(vx, dx, ax, &t0, &t1);
    gpd_ray_slab(vy, dy, ay, &t0, &t1);
    gpd_ray_slab(vz, dz, az, &t0, &t1);
    return t0 <= t1 ? t0 : GPD_OBST_INF;
}

/* vertical cylinder: the infinite cylinder's interval (the quadratic in the x-y plane, a = dx^2 + dy^2; a vertical ray decides by
 * its distance from the axis) intersected with the slab of the caps */
GPD_HOST_DEVICE static inline float gpd_ray_cylinder(float vx, float vy, float vz, float dx, float dy, float dz, float r, float h) {
    float t0 = 0.0f, t1 = GPD_OBST_INF;
    const float a = dx * dx + dy * dy;
    const float c = (vx * vx + vy * vy) - r * r;
    if (a == 0.0f) {
        if (c > 0.0f) return GPD_OBST_INF;
    } else {
        const float bh = (vx * dx + vy * dy) / a;        /* the closest approach to the axis is at t = -bh */
        const float px = vx - bh * dx, py = vy - bh * dy;
        const float disc = r * r - (px * px + py * py);
        if (!(disc >= 0.0f)) return GPD_OBST_INF;
        const float half = sqrtf(disc / a);
        const float t_out = half - bh;
        const float t_in = (c > 0.0f && t_out > 0.0f) ? (c / a) / t_out : -bh - half;      /* (no cancellation for an origin outside) */
        t0 = fmaxf(t0, t_in);
        t1 = fminf(t1, t_out);
    }
    gpd_ray_slab(vz, dz, h, &t0, &t1);
    return t0 <= t1 ? t0 : GPD_OBST_INF;
}

/* the half-space z <= 0 (relative to the record's cz): only a descending ray enters it */
GPD_HOST_DEVICE static inline float gpd_ray_floor(float vz, float dz) {
    if (!(vz > 0.0f)) return 0.0f;
    return dz < 0.0f ? vz / -dz : GPD_OBST_INF;
}

GPD_HOST_DEVICE static inline float gpd_obst_ray(int kind, float ax, float ay, float az, float vx, float vy, float vz, float dx, float dy,
                                                 float dz) {
    switch (kind) {
    case GPD_OBST_SPHERE: return gpd_ray_sphere(vx, vy, vz, dx, dy, dz, ax);
    case GPD_OBST_BOX: return gpd_ray_box(vx, vy, vz, dx, dy, dz, ax, ay, az);
    case GPD_OBST_CYLINDER: return gpd_ray_cylinder(vx, vy, vz, dx, dy, dz, ax, az);
    case GPD_OBST_FLOOR: return gpd_ray_floor(vz, dz);
    default: return GPD_OBST_INF;
    }
}

#endif
