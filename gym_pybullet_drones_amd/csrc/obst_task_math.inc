/* obst_task_math.inc -- how gpd_rollout_obst (include/gpd.h) combines the task's reward with the clearance of the pose a step reached.
 * Plain C, on purpose, as obstacle_math.inc and mppi_math.inc are: the kernel in obst_task.inc and the host program
 * tests/c/obst_task_host.c compile THIS text, so the formula a machine without a GPU holds against the float64 restatement
 * (tests/helpers/obst_task_f64.py) is the one the device runs.  Every operation is a separate IEEE fp32 one (no fused multiply-add),
 * so elementwise fp32 arithmetic in any other place gives the same bits.  Included after gpd.h. */
#ifndef GPD_OBST_TASK_MATH_INC
#define GPD_OBST_TASK_MATH_INC

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_OT_HOST_DEVICE __host__ __device__
#else
#include <math.h>
#define GPD_OT_HOST_DEVICE
#pragma clang fp contract(off)      /* as the device build (-ffp-contract=off): the host rounds what the kernel rounds */
#endif

/* contact: the drone, a sphere of radius r, reaches into the nearest obstacle (strictly; false for d = +inf) */
GPD_OT_HOST_DEVICE static inline int gpd_obst_task_hit(float d, float collision_radius) { return d < collision_radius; }

/* the proximity hinge max(0, prox_margin - (d - r)): how far the gap to contact is inside the margin; 0 for d = +inf */
GPD_OT_HOST_DEVICE static inline float gpd_obst_task_hinge(float d, float collision_radius, float prox_margin) {
    const float gap = d - collision_radius;
    return fmaxf(0.0f, prox_margin - gap);
}

/* reward = task_reward + hit_reward * hit - prox_weight * hinge: at most five roundings (gap, margin - gap, the product, the sum
 * with hit_reward -- taken only in contact -- and the difference) */
GPD_OT_HOST_DEVICE static inline float gpd_obst_task_reward(float task_reward, float d, float collision_radius, float hit_reward,
                                                            float prox_margin, float prox_weight) {
    const float base = gpd_obst_task_hit(d, collision_radius) ? task_reward + hit_reward : task_reward;
    const float pen = prox_weight * gpd_obst_task_hinge(d, collision_radius, prox_margin);
    return base - pen;
}

#endif
