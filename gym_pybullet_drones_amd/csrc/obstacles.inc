// obstacles.inc -- gpd_obstacles (include/gpd.h): clearance, collisions and range scans against a list of analytic obstacles.
// Pulled into abi.hip; the geometry is obstacle_math.inc, the text a host program compiles too.  DESIGN.md section 3.14.
//
// Two kernels, one launch each, no atomics, one writer per word:
//   obst_clear_kernel  one lane per drone: the minimum over the records of each one's signed distance, that record and its gradient
//   obst_scan_kernel   one lane per (drone, ray), the ray index fastest: a wave stores 256 contiguous bytes of `ranges`, and the lanes
//                      of a drone read one pose address
// SHARED (obst_ld = 1): the workgroup stages the list into LDS once (n_obst x 32 bytes, at most 32 KiB) and every lane walks it at the
// same index -- one ds_read_b128 pair per record whose address is wave-uniform (a broadcast, no bank conflict), and the record's kind
// goes through v_readfirstlane so that the branch on it is a scalar one: a wave evaluates ONE shape per record.
// Per-aviary lists (field planes, float f of record m of aviary e at obst[(m * 8 + f) * ld + e]) are read from global memory: with
// D = 1 neighbouring lanes read neighbouring aviaries, coalesced, but their kinds may differ, so the shapes are evaluated under the
// lane's predicate -- a wave pays for every kind that occurs among its 64 records at that m.
#include "obstacle_math.inc"

namespace {

struct ObstRecord { float cx, cy, cz, ax, ay, az; int kind; };

// the record's kind from its float; a NaN is no kind (GPD_OBST_NONE)
__device__ __forceinline__ int obst_kind(float w) { return w == w ? static_cast<int>(w) : GPD_OBST_NONE; }

template <bool SHARED>
__device__ __forceinline__ void obst_stage(const float* __restrict__ obst, int n_obst, float4* lds) {
    if constexpr (SHARED) {
        float* dst = reinterpret_cast<float*>(lds);                      // [n_obst][8] floats, contiguous in global memory too
        for (int k = threadIdx.x; k < GPD_OBST_FLOATS * n_obst; k += kBlock) dst[k] = obst[k];
        __syncthreads();
    }
}

template <bool SHARED>
__device__ __forceinline__ ObstRecord obst_record(const float* __restrict__ obst, const float4* lds, int m, int64_t ld, int64_t e) {
    ObstRecord r;
    if constexpr (SHARED) {
        const float4 a = lds[2 * m], b = lds[2 * m + 1];
        r.cx = a.x; r.cy = a.y; r.cz = a.z; r.ax = b.x; r.ay = b.y; r.az = b.z;
        r.kind = __builtin_amdgcn_readfirstlane(obst_kind(a.w));      // (the same word in every lane: makes the branch scalar)
    } else {
        const float* p = obst + static_cast<int64_t>(m) * GPD_OBST_FLOATS * ld + e;
        r.cx = p[0]; r.cy = p[ld]; r.cz = p[2 * ld]; r.ax = p[4 * ld]; r.ay = p[5 * ld]; r.az = p[6 * ld];
        r.kind = obst_kind(p[3 * ld]);
    }
    return r;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return (fabsf(x) < GPD_OBST_INF) & (fabsf(y) < GPD_OBST_INF) & (fabsf(z) < GPD_OBST_INF);      // (false for NaN)
}

// a ray direction of the table turned into the world frame by the attitude q (GPD_RAY_BODY: |q| does not matter) or by its yaw alone
// (GPD_RAY_LEVEL: the yaw of pybullet's Euler angles of the normalised quaternion); GPD_RAY_WORLD leaves it.  `frame` is wave-uniform.
// Shared by obst_scan_kernel and the fused task kernel (obst_task.inc): one text, the same bits.
__device__ __forceinline__ void obst_turn_ray(int frame, float qx, float qy, float qz, float qw, float& dx, float& dy, float& dz) {
    if (frame == GPD_RAY_BODY) {
        const Mat3 R = quat_to_mat(qx, qy, qz, qw);
        const float bx = dx, by = dy, bz = dz;
        dx = fmaf(R.r02, bz, fmaf(R.r01, by, R.r00 * bx));
        dy = fmaf(R.r12, bz, fmaf(R.r11, by, R.r10 * bx));
        dz = fmaf(R.r22, bz, fmaf(R.r21, by, R.r20 * bx));
    } else if (frame == GPD_RAY_LEVEL) {
        const float s = fast_rsq(fmaf(qx, qx, fmaf(qy, qy, fmaf(qz, qz, qw * qw))));
        float roll, pitch, yaw, sy, cy;
        quat_to_rpy(qx * s, qy * s, qz * s, qw * s, roll, pitch, yaw);
        sy = sinf(yaw); cy = cosf(yaw);
        const float bx = dx, by = dy;
        dx = fmaf(cy, bx, -(sy * by));
        dy = fmaf(sy, bx, cy * by);
    }
}

template <bool SHARED>
__global__ __launch_bounds__(kBlock) void obst_clear_kernel(const float4* __restrict__ pos4, int n, int D, const float* __restrict__ obst,
                                                            int n_obst, int64_t ld, float collision_radius, float4* __restrict__ clear4,
                                                            int32_t* __restrict__ nearest, uint8_t* __restrict__ hit) {
    extern __shared__ __attribute__((aligned(16))) float4 obst_lds[];
    obst_stage<SHARED>(obst, n_obst, obst_lds);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = pos4[i];
    const int64_t e = SHARED ? 0 : i / D;
    float best = GPD_OBST_INF, bx = 0.0f, by = 0.0f, bz = 0.0f;
    int who = -1;
    if (finite3(p.x, p.y, p.z)) {
        for (int m = 0; m < n_obst; ++m) {
            const ObstRecord r = obst_record<SHARED>(obst, obst_lds, m, ld, e);
            float nx, ny, nz;
            const float d = gpd_obst_sdf(r.kind, r.ax, r.ay, r.az, p.x - r.cx, p.y - r.cy, p.z - r.cz, &nx, &ny, &nz);
            const bool closer = d < best;            // (strict: a tie keeps the lower m; false for a NaN from a record that is not finite)
            best = closer ? d : best;
            bx = closer ? nx : bx; by = closer ? ny : by; bz = closer ? nz : bz;
            who = closer ? m : who;
        }
    }
    if (clear4) clear4[i] = make_float4(bx, by, bz, best);
    if (nearest) nearest[i] = who;
    if (hit) hit[i] = best < collision_radius ? 1 : 0;
}

template <bool SHARED>
__global__ __launch_bounds__(kBlock) void obst_scan_kernel(const float4* __restrict__ pos4, const float4* __restrict__ quat4, int n, int D,
                                                           const float* __restrict__ obst, int n_obst, int64_t ld,
                                                           const float* __restrict__ ray_dirs, int n_rays, int frame, float max_range,
                                                           float* __restrict__ ranges, int32_t* __restrict__ ray_hit) {
    extern __shared__ __attribute__((aligned(16))) float4 obst_lds[];
    obst_stage<SHARED>(obst, n_obst, obst_lds);
    const uint32_t j = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;        // (n * n_rays <= 2^32 and at most 2^24 workgroups)
    const uint32_t i = j / static_cast<uint32_t>(n_rays);
    if (i >= static_cast<uint32_t>(n)) return;
    const int ray = static_cast<int>(j - i * static_cast<uint32_t>(n_rays));
    const float4 p = pos4[i];
    const int64_t e = SHARED ? 0 : i / static_cast<uint32_t>(D);
    float dx = ray_dirs[3 * ray], dy = ray_dirs[3 * ray + 1], dz = ray_dirs[3 * ray + 2];
    if (frame != GPD_RAY_WORLD) {              // (wave-uniform)
        const float4 q = quat4[i];
        obst_turn_ray(frame, q.x, q.y, q.z, q.w, dx, dy, dz);
    }
    float best = max_range;
    int who = -1;
    if (finite3(p.x, p.y, p.z) && finite3(dx, dy, dz)) {
        for (int m = 0; m < n_obst; ++m) {
            const ObstRecord r = obst_record<SHARED>(obst, obst_lds, m, ld, e);
            const float t = gpd_obst_ray(r.kind, r.ax, r.ay, r.az, p.x - r.cx, p.y - r.cy, p.z - r.cz, dx, dy, dz);
            const bool closer = t < best;            // (strict: ties keep the lower m; an entry AT max_range is no hit)
            best = closer ? t : best;
            who = closer ? m : who;
        }
    }
    ranges[j] = best;
    if (ray_hit) ray_hit[j] = who;
}

}  // namespace

extern "C" int gpd_obstacles(const float* pos4, const float* quat4, int32_t n, int32_t drones_per_env, const float* obst, int32_t n_obst,
                             int64_t obst_ld, float collision_radius, float* clear4, int32_t* nearest, uint8_t* hit, const float* ray_dirs,
                             int32_t n_rays, int32_t ray_frame, float max_range, float* ranges, int32_t* ray_hit, void* stream) {
    const Refuse bad{"gpd_obstacles"};
    const int32_t D = drones_per_env;
    if (!pos4 || !obst) return bad(GPD_EINVAL, "NULL pos4/obst");
    if (!clear4 && !nearest && !hit && !ranges) return bad(GPD_EINVAL, "no output: one of clear4, nearest, hit, ranges must be given");
    if (misaligned16(pos4) || misaligned16(quat4) || misaligned16(clear4)) return bad(GPD_EINVAL, "pos4, quat4 and clear4 must be 16-byte aligned");
    if (n <= 0 || D < 0 || (D > 0 && n % D != 0)) return bad(GPD_EINVAL, "n must be positive and a multiple of drones_per_env (>= 0)");
    if (n > (1 << 26)) return bad(GPD_ERANGE, "more than 2^26 drones per launch");
    if (n_obst < 1 || n_obst > GPD_OBST_MAX) return bad(GPD_ERANGE, "n_obst must be in 1..1024");
    const bool shared = obst_ld == 1;
    if (!shared && (D == 0 || obst_ld < n / D)) return bad(GPD_EINVAL, "obst_ld must be 1 (one shared list) or >= n / drones_per_env (one list per aviary, drones_per_env >= 1)");
    if (ranges) {
        if (!ray_dirs) return bad(GPD_EINVAL, "ranges needs ray_dirs");
        if (n_rays < 1 || n_rays > GPD_OBST_MAX_RAYS) return bad(GPD_ERANGE, "n_rays must be in 1..64");
        if (ray_frame < GPD_RAY_WORLD || ray_frame > GPD_RAY_BODY) return bad(GPD_EINVAL, "unknown ray_frame");
        if (!(max_range > 0.0f) || !(max_range < GPD_OBST_INF)) return bad(GPD_EINVAL, "max_range must be positive and finite");
        if (ray_frame != GPD_RAY_WORLD && !quat4) return bad(GPD_EINVAL, "ray_frame LEVEL / BODY needs quat4");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = shared ? static_cast<size_t>(n_obst) * GPD_OBST_FLOATS * sizeof(float) : 0;
    const float4* P = reinterpret_cast<const float4*>(pos4);
    const int Dk = D > 0 ? D : n;              // (one world: every row in aviary 0)
    if (clear4 || nearest || hit) {
        auto launch = [&](auto SH) {
            hipLaunchKernelGGL(obst_clear_kernel<decltype(SH)::value>, dim3(blocks_for(n, kBlock)), dim3(kBlock), lds, st, P, n, Dk, obst, n_obst,
                               obst_ld, collision_radius, reinterpret_cast<float4*>(clear4), nearest, hit);
        };
        if (shared) launch(Const<true>{}); else launch(Const<false>{});
        if (int rc = launched(bad.who, " (clearance) launch")) return rc;
    }
    if (ranges) {
        auto launch = [&](auto SH) {
            hipLaunchKernelGGL(obst_scan_kernel<decltype(SH)::value>, dim3(blocks_for(static_cast<int64_t>(n) * n_rays, kBlock)), dim3(kBlock), lds,
                               st, P, reinterpret_cast<const float4*>(quat4), n, Dk, obst, n_obst, obst_ld, ray_dirs, n_rays, ray_frame,
                               max_range, ranges, ray_hit);
        };
        if (shared) launch(Const<true>{}); else launch(Const<false>{});
        if (int rc = launched(bad.who, " (scan) launch")) return rc;
    }
    return 0;
}
