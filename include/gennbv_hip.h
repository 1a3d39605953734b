/*
 * gennbv_hip.h -- C-ABI of libgennbv_hip.so, the MI355X (gfx950) implementation of
 * GenNBV's state-encoding + PPO hot path.
 *
 * Conventions (SURVEY.md section 8b "Ownership / lifetime"):
 *   - every pointer is a CALLER-OWNED DEVICE pointer (HBM) unless marked [host];
 *     nothing is retained or freed; scratch comes from a caller-owned workspace;
 *   - `stream` is the caller's hipStream_t passed as void* (NULL = default stream);
 *     all work is enqueued on it, nothing synchronises the device;
 *   - return value: 0 on success, otherwise a hipError_t value
 *     (1 = hipErrorInvalidValue for bad arguments). Never throws.
 *   - tensors are dense row-major fp32 unless stated; grids are [N, G, G, G]
 *     C-order over (X, Y, Z) exactly like the reference's torch tensors.
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * the zjwzcx/GenNBV root). INTEGRATION.md shows the ctypes binding a maintainer
 * would add on the reference side.
 */
#ifndef GENNBV_HIP_H
#define GENNBV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNBV_ABI_VERSION 5

int gnbv_abi_version(void);
/* Name of the device architecture the library was compiled for ("gfx950"). [host] */
const char *gnbv_build_arch(void);

/* ------------------------------------------------------------------------- */
/* A1  Env_Train_Base.post_process_camera_tensor, depth + seg branch          */
/*     gennbv/env/env_train_base.py:521-534                                    */
/* ------------------------------------------------------------------------- */
int gnbv_post_process_depth(const float *depth_raw, const float *seg_raw, int64_t count,
                            float depth_sense_dist, float *depth_out, float *seg_out, void *stream);

/* A1 rgb branch (env_train_base.py:517-520): RGBA u8 [N,H,W,4] -> nearest
 * resize to [oh,ow] -> grayscale f32 [N,1,oh,ow].  Parity unpinned (torchvision). */
int gnbv_rgb_to_gray(const uint8_t *rgba, int n, int h, int w, int oh, int ow, float *gray,
                     int64_t gray_row_stride /* floats between envs, >= oh*ow */, void *stream);

/* ------------------------------------------------------------------------- */
/* A2  Env_Train_GenNBV.back_projection_fg  (env_train_gennbv.py:494-533)      */
/*     depth/seg are the PROCESSED tensors; c2w [N,4,4] is inv(view^T) @        */
/*     blender2opencv with env_origins subtracted (host plumbing, :512-514).   */
/*     world [N,HW,3]; fg [N,HW] u8 (seg > 50).                                 */
/* ------------------------------------------------------------------------- */
int gnbv_back_projection(const float *depth, const float *seg, const float *c2w, const float *inv_intri /*[host] [3,3]*/,
                         int n, int h, int w, float *world, uint8_t *fg, void *stream);

/* A3  scanned_pts_to_idx_3D (gennbv/utils.py:230-270), per point, before the
 *     set reduction: idx [N,HW,3] int32, (-1,-1,-1) for dropped points. */
int gnbv_points_to_idx(const float *world, const uint8_t *fg, const float *range_gt /*[N,6]*/,
                       const float *voxel_size /*[N,3]*/, int n, int64_t hw, int g, int32_t *idx, void *stream);

/* A4  pose_coord_to_idx_3D (gennbv/utils.py:273-306, if_col=False): no clamp. */
int gnbv_pose_to_idx(const float *poses_xyz /*[N,3]*/, const float *range_gt, const float *voxel_size, int n,
                     int64_t *pose_idx /*[N,3]*/, void *stream);

/* A5  bresenham3D_pycuda kernel launch (gennbv/utils.py:170-220): one source,
 *     num_rays targets; trajectory_pts [num_rays, 3*map_size, 3] int32 and
 *     trajectory_lengths [num_rays] int32 must be zero-filled by the caller
 *     (as utils.py:40-41 does). */
int gnbv_bresenham3d(const int32_t *source_pts /*[3]*/, const int32_t *target_pts /*[R,3]*/, int num_rays, int map_size,
                     int32_t *trajectory_pts, int32_t *trajectory_lengths, void *stream);

/* A7  grid_occupancy_tri_cls (gennbv/utils.py:309-325), return_tri_cls_only. */
int gnbv_grid_tri_cls(const float *grid_prob, int64_t count, float threshold_occu, float threshold_free,
                      float *grid_tri_cls, void *stream);

/* ------------------------------------------------------------------------- */
/* A1-A7 fused: Env_Train_GenNBV.update_occ_grid (env_train_gennbv.py:277-326)  */
/*   One call = one environment step for all N envs, three launches:           */
/*     hit-mask scatter (LDS-staged bitmask) -> ray cast (LDS path bitmask)     */
/*     -> streaming grid update.                                                */
/*   depth_raw / seg_raw are the RAW camera tensors (A1 is fused).  When        */
/*   w % 4 == 0 (and h*w < 2^23) the kernels fetch four pixels of a row per     */
/*   16-byte request: both pointers must then be 16-byte aligned, a call with   */
/*   another pointer is refused (all three entry points; no other argument is   */
/*   fetched wider than its element unless the call has checked its alignment). */
/*   A refused call (non-zero return for an argument) launches nothing and      */
/*   leaves the workspace as it was.                                            */
/*   reset_mask [N] u8 or NULL: env rows whose prob/scanned grids are treated   */
/*   as zero before the update (reset_idx :416-420 folded into the next step).  */
/*   tri_out: row e starts at tri_out + e*tri_row_stride (floats) so the        */
/*   tri-class grid can land directly inside the flat observation row           */
/*   (wrapper key order state, grid, state_rgb).                                */
/*   coverage_count [N] int32 = number of non-zero scanned_gt voxels            */
/*   (== scanned_gt.sum() for the reference's binary GT, :537).                 */
/*   workspace: gnbv_voxel_workspace_bytes(n, g) bytes, 256-byte aligned.       */
/* ------------------------------------------------------------------------- */
size_t gnbv_voxel_workspace_bytes(int n, int g);
/* The same two bitmask arrays + per-env ray lists (one int32 per distinct hit voxel and image chunk, capacity h*w per
 * env): with a workspace of at least this size the update runs the hit-list + load-balanced ray-cast launches
 * (csrc/voxel.hip: k_hit_list, k_ray_list; grids whose hit mask, word list and pixel queue do not fit a workgroup's 160 KiB of LDS
 * together -- G > 93 -- k_hit_atomic, k_ray_slab); with
 * the smaller mask-only workspace it falls back to k_hit_mask + k_raycast.
 * Same results either way. */
size_t gnbv_voxel_workspace_bytes_hw(int n, int g, int h, int w);
/* gnbv_update_occ_grid_coded, workspace_flags: the caller guarantees that the two mask arrays and the ray counts of the
 * workspace are ZERO on entry -- freshly zero-initialised, or left so by the previous call made with this flag -- and the
 * call leaves them zero (its grid-update launch clears every word it consumes): the 16 MB fill launch per call goes away.
 * Do not set it on a workspace that another entry point (or a call without the flag) has used since. */
#define GNBV_VOXEL_WS_CLEAN 1

int gnbv_update_occ_grid(const float *depth_raw, const float *seg_raw, const float *c2w,
                         const float *inv_intri /*[host] [3,3]*/,
                         const float *poses_xyz /*[N,3]*/, int64_t poses_row_stride /*floats*/,
                         const float *range_gt, const float *voxel_size, const float *grid_gt,
                         const uint8_t *reset_mask, int n, int h, int w, int g, float depth_sense_dist,
                         float *prob_grid, float *scanned_gt_grid, float *tri_out, int64_t tri_row_stride,
                         int32_t *coverage_count, void *workspace, size_t workspace_bytes, void *stream);

/* Packed variant of gnbv_update_occ_grid for a BINARY ground truth (the reference's GT is an
 * occupancy indicator): grid_gt and scanned_gt_grid are bitmasks [N, gnbv_grid_bit_words(G)] u32
 * (bit v = voxel (x*G+y)*G+z). scanned = clip(scanned + occ*gt, 0, 1) == scanned | (hit & gt)
 * exactly, coverage = popcount. Identical results, half the HBM traffic of the streaming pass. */
int gnbv_grid_bit_words(int g);
int gnbv_pack_grid_bits(const float *grid /*[N,G^3]*/, int n, int g, uint32_t *bits, int *not_binary /*[1] or NULL*/,
                        void *stream);
int gnbv_unpack_grid_bits(const uint32_t *bits, int n, int g, float *grid /*[N,G^3] of {0,1}*/, void *stream);
int gnbv_update_occ_grid_packed(const float *depth_raw, const float *seg_raw, const float *c2w,
                                const float *inv_intri /*[host] [3,3]*/, const float *poses_xyz, int64_t poses_row_stride,
                                const float *range_gt, const float *voxel_size, const uint32_t *gt_bits,
                                const uint8_t *reset_mask, int n, int h, int w, int g, float depth_sense_dist,
                                float *prob_grid, uint32_t *scanned_bits, float *tri_out, int64_t tri_row_stride,
                                int32_t *coverage_count, void *workspace, size_t workspace_bytes, void *stream);

/* Debug/parity view of the workspace after gnbv_update_occ_grid: expands the
 * hit / path bitmasks to u8 [N,G^3] (either output may be NULL). */
int gnbv_unpack_masks(const void *workspace, int n, int g, uint8_t *hit_u8, uint8_t *path_u8, void *stream);

/* Coded probability grid (same A1-A7 step, 1 byte per voxel instead of an fp32 prob_grid): between two resets a voxel's
 * probability is a function of (base, k) -- base = 1 after a hit (prob = 1.0, env_train_gennbv.py:311) / 0 since the
 * reset, k = number of "prob -= 0.05" path steps since (:308) -- so code = base << 7 | k is exact for episodes of at
 * most 127 steps (*overflow is set to 1 if a counter saturates).  gnbv_prob_code_tables fills the 256-entry HOST
 * tables prob_lut[code] (the exact fp32 iteration) and tri_lut[code] (A7); pass DEVICE copies to the kernels. */
void gnbv_prob_code_tables(float *prob_lut /*[256] host or NULL*/, float *tri_lut /*[256] host or NULL*/);
int gnbv_decode_prob_grid(const uint8_t *prob_code, int64_t count, const float *prob_lut /*[256] device*/, float *prob_out,
                          void *stream);
int gnbv_update_occ_grid_coded(const float *depth_raw, const float *seg_raw, const float *c2w, const float *inv_intri /*[host]*/,
                               const float *poses_xyz, int64_t poses_row_stride, const float *range_gt, const float *voxel_size,
                               const uint32_t *gt_bits, const uint8_t *reset_mask, int n, int h, int w, int g,
                               float depth_sense_dist, uint8_t *prob_code /*[N,G^3]*/, const float *tri_lut /*[256] device*/,
                               uint32_t *scanned_bits, float *tri_out /*NULL: compact observations, int8 rows only*/,
                               int64_t tri_row_stride,
                               int8_t *tri_i8 /*NULL, or the tri-class grid as int8 rows (-1/0/1): row e at tri_i8 + e*stride;
                                                at least one of tri_out / tri_i8 must be given*/,
                               int64_t tri_i8_row_stride /*bytes*/, int32_t *coverage_count,
                               int32_t *overflow /*[1] device or NULL*/, void *workspace, size_t workspace_bytes,
                               int workspace_flags /* GNBV_VOXEL_WS_* */, void *stream);


/* ------------------------------------------------------------------------- */
/* A8/A9  environment-step bookkeeping (no simulator: recorded/synthetic feed)  */
/* ------------------------------------------------------------------------- */
/* Action lattice of the task (gennbv/env/config_gennbv_train.py:62-69). [host struct] */
typedef struct GnbvLattice {
    int64_t clip_low[6], clip_up[6], init_action[6];
    float action_unit[6], pose_low[6], init_pose[6];
} GnbvLattice;

/* Env_Train_GenNBV.step head (env_train_gennbv.py:246-255) + post_physics_step's
 * episode_length_buf += 1 (:337): clip actions, force init_action where
 * episode_length_buf == 0, poses = action*unit + low. actions int64 [N,6], poses f32 [N,6]. */
int gnbv_env_pre_step(const int64_t *actions_in, const GnbvLattice *lattice /*[host]*/, int64_t *episode_length_buf,
                      int n, int64_t *actions_out, float *poses_out, void *stream);

/* update_obs_buf pose deque (:273-275) + obs["state"] (:361): pose_hist [N,stack,6]
 * oldest->newest is shifted, the new pose appended, and the row is written to
 * obs + e*obs_row_stride. reset_mask [N] (may be NULL): history was refilled with
 * init_pose_buf by reset_idx (:397-400). */
int gnbv_env_obs_state(float *pose_hist, const float *poses, const uint8_t *reset_mask, const GnbvLattice *lattice /*[host]*/,
                       int n, int stack, float *obs, int64_t obs_row_stride, void *stream);

/* post_process_camera_tensor rgb branch (env_train_base.py:517-520) + rgb deque (k=2)
 * + obs["state_rgb"] (:363): writes [older | newest] gray frames (2*oh*ow floats) at
 * obs_rgb + e*obs_row_stride; gray_prev [N,oh*ow] is the persistent older frame. */
int gnbv_env_obs_rgb(const uint8_t *rgba, float *gray_prev, const uint8_t *reset_mask, int n, int h, int w, int oh, int ow,
                     float *obs_rgb, int64_t obs_row_stride, void *stream);

/* The three calls above as ONE launch (round 5; a new entry point of ABI 5, no layout changes): same arguments, same arithmetic, bit-identical outputs -- what a reference-side integration
 * would issue between `step(actions)` and `update_occ_grid` (env_train_gennbv.py:246-275).  obs_rgb = the row's state_rgb slice (same
 * row stride as obs). */
int gnbv_env_observe(const int64_t *actions_in, const GnbvLattice *lattice /*[host]*/, int64_t *episode_length_buf, int n, int64_t *actions_out,
                     float *poses_out, float *pose_hist, const uint8_t *reset_mask, int stack, float *obs, int64_t obs_row_stride,
                     const uint8_t *rgba, float *gray_prev, int h, int w, int oh, int ow, float *obs_rgb, void *stream);

/* Closed-loop camera (a new entry point of ABI 5): renders every env from the pose step() computed, in place of the
 * Isaac Gym camera sensors (env_train_gennbv.py:346-354).  The scene is a triangle soup per env (env-local frame, the
 * frame of the poses and range_gt) with a uniform cell grid of conservative triangle lists (CSR), built once by
 * gennbv_amd/env/mesh_scene.py.  [host struct]; every pointer in it is device.
 *
 * The grid contract, for a caller that builds the arrays itself.  Every kernel that takes a scene (gnbv_render_depth,
 * gnbv_view_cover[_masks], gnbv_voxelize_surface, gnbv_collide_cylinder[_batch], gnbv_sweep_sphere) asks one thing of the
 * lists: they are conservative (below).  Its outputs then do not depend on which conservative grid it is given -- box,
 * resolution, list order, layout: the same bits (tests/test_mesh_grids_gpu.py; rgba alone may differ where two triangles
 * of different objects tie exactly for the closest hit, because the first one visited wins).
 *   - A cell's list may be in any order and may repeat a triangle.  (The voxelizer looks a triangle up in neighbouring
 *     cells by binary search only to skip duplicate work; on an unsorted list the search misses and the triangle is
 *     tested again, the results are ORed.)
 *   - A list may name triangles that do not touch its cell, up to every triangle of the env in every cell; it may only
 *     name triangles of its own env.  Cost grows with the lists, the result does not change.
 *   - The box [cell_lo, cell_lo + cell_res * cell_size] must hold every vertex of the env strictly inside; beyond that it
 *     may be any size and lie anywhere (around the cameras, below z = 0), cell_res may be 1 on any axis and the cell edges
 *     may differ between axes (tested up to 1024 cells on an axis).
 *   - The cell blocks of the envs may lie anywhere in cell_start, in any order, with unused cells (empty lists) between
 *     them.  cell_base of an env with cell_res 0 indexes nothing.
 *   - Conservative means the builder's rule (MeshScene._bin): a triangle is listed in every cell that its axis-aligned
 *     bounding box, grown on every side by eps = 1e-4 * L + 1e-5 m, overlaps, with the cell index
 *     floor((x - cell_lo) / cell_size) taken in fp32 and clamped to the grid.  L = the largest extent of the env's triangle
 *     bounds; a box much larger than the triangles takes its own largest extent, because the rounding below grows with the
 *     box.  The exact overlap alone is not enough: the renderer walks the cells in fp32 and adds one rounded step per cell
 *     crossed, so a boundary crossing it computes lies up to 3.5e-4 m (measured at 1024 cells on an axis of 19 m,
 *     tests/test_mesh_grids_cpu.py) from the true one; eps is 1.9e-3 m there. */
typedef struct GnbvMeshScene {
    int n;                          /* envs */
    const float *tris;              /* [T,3,3] triangle vertices, all envs concatenated (NULL if T == 0) */
    const int32_t *tri_obj;         /* [T] object id of each triangle, > 0 */
    const float *cell_lo;           /* [N,3] lower corner of the env's cell grid */
    const float *cell_size;         /* [N,3] cell edge per axis */
    const int32_t *cell_res;        /* [N,3] cells per axis (x fastest); 0,0,0 = an env without triangles */
    const int32_t *cell_base;       /* [N] global index of the env's first cell */
    const int32_t *cell_start;      /* [cells + 1] CSR offsets into cell_tris */
    const int32_t *cell_tris;       /* triangle indices into tris (NULL if empty) */
} GnbvMeshScene;

/* c2w [N,4,4] from poses (x, y, z, roll, pitch, yaw) in synthetic.camera_to_world's convention (fp64 trig rounded to
 * fp32, roll ignored), then one ray per pixel d = R * inv_intri * (u, v, 1) cast against the env's triangles and the
 * ground plane z = 0: depth_raw [N,H,W] = -t (-inf on a miss), seg_raw [N,H,W] = 255 on an object / 0 on ground or
 * miss, rgba [N,H,W,4] u8 (NULL: none) = synthetic.render_depth's shading of the hit's object id.  Deterministic. */
int gnbv_render_depth(const GnbvMeshScene *scene /*[host]*/, const float *poses, int64_t poses_row_stride /*floats*/,
                      const float *inv_intri /*[host] [3,3]*/, int h, int w, float *c2w_out, float *depth_raw, float *seg_raw,
                      uint8_t *rgba, void *stream);

/* Ground truth from the same triangles (a new entry point of ABI 5): surface voxelization of every env of the scene
 * under the updater's voxel bounds (gnbv_pose_to_idx): per axis v = voxel_size[a], vmin = fp32(range_min[a] - fp32(0.5 * v)),
 * voxel i = the closed interval [vmin + i*v, vmin + (i+1)*v] in fp64.  grid_out [N,g,g,g] = 1.0 where the voxel's closed
 * box meets a closed triangle of the env (a degenerate triangle counts as its segment or point), 0.0 elsewhere.  Every
 * voxel is written (no zero fill needed); deterministic.  Against the exact answer: no false negatives, and a false
 * positive only within 2^-36 * (largest |coordinate| of the triangle and the voxel) of the triangle.  range_gt [N,6] and
 * voxel_size [N,3] are device arrays: an env whose voxel size is not positive and finite cannot be refused without a
 * host sync, so its grid is filled with NaN.  g outside 2..1024 or a bad scene returns hipErrorInvalidValue. */
int gnbv_voxelize_surface(const GnbvMeshScene *scene /*[host]*/, const float *range_gt /*[N,6]*/, const float *voxel_size /*[N,3]*/,
                          int g, float *grid_out /*[N,g,g,g] f32*/, void *stream);

/* Collision termination (a new entry point of ABI 5): does the drone body of each env meet that env's scene?  The body is
 * a closed solid cylinder of radius `radius` and half-length `half_length` (cf2x.urdf base_link: 0.1, 0.02) centred at the
 * pose's (x, y, z), axis a = R e_z, R = Rz(yaw) Ry(pitch) Rx(roll) evaluated in fp64 from the fp32 poses.  Every object of an env
 * (a MeshScene object id) is a closed solid: its triangles plus the points of its closed AABB where the generalized winding
 * number of its triangles has |w| >= 1/2 (for a closed, consistently wound mesh: interior and surface).  The per-object index
 * is built once by gennbv_amd/env/mesh_scene.py (MeshScene.objects).  [host struct]; every pointer in it is device. */
typedef struct GnbvMeshObjects {
    int n;                          /* envs, == GnbvMeshScene.n */
    int num_objects;                /* K, all envs */
    const int32_t *env_obj_start;   /* [N+1] CSR: the objects of env e are env_obj_start[e] .. env_obj_start[e+1] - 1 */
    const float *obj_aabb;          /* [K,6] closed AABB of each object's triangles: xmin, ymin, zmin, xmax, ymax, zmax (NULL if K == 0) */
    const int32_t *obj_tri_start;   /* [K+1] CSR offsets into obj_tris */
    const int32_t *obj_tris;        /* the triangle indices (into GnbvMeshScene.tris) of each object (NULL if K == 0) */
} GnbvMeshObjects;

/* contact_out[e] = bit 0 (S): a triangle of env e meets the solid cylinder (one entirely inside it included) | bit 1 (I): (S)
 * is false and the centre lies in an object's solid | bit 2 (G): ground != 0 and the body's lowest point
 * z - (radius sqrt(1 - a_z^2) + half_length |a_z|) is <= 0.  0 = free.  poses [N, >= 6] (x, y, z, roll, pitch, yaw) with a row
 * stride in floats; an env with a non-finite pose gets 0.  Deterministic (no atomics).  radius > 0 and half_length >= 0
 * finite, a scene and an index of the same envs, else hipErrorInvalidValue. */
int gnbv_collide_cylinder(const GnbvMeshScene *scene /*[host]*/, const GnbvMeshObjects *objects /*[host]*/, const float *poses,
                          int64_t poses_row_stride /*floats*/, float radius, float half_length, int ground, uint8_t *contact_out /*[N]*/,
                          void *stream);
/* K candidate poses per env in one launch (one wave per (env, candidate)): contact_out[e, j] is bit-identical to what
 * gnbv_collide_cylinder stores for env e at pose (e, j).  poses [N, K, >= 6] with the stride between consecutive (e, j) rows in
 * floats; k >= 1, N * k <= 2^31 - 1, else as gnbv_collide_cylinder. */
int gnbv_collide_cylinder_batch(const GnbvMeshScene *scene /*[host]*/, const GnbvMeshObjects *objects /*[host]*/, const float *poses,
                                int k, int64_t poses_row_stride /*floats*/, float radius, float half_length, int ground,
                                uint8_t *contact_out /*[N,K]*/, void *stream);

/* Swept flight path (a new entry point of ABI 5): does the drone, flown straight from one pose to the next, meet the scene?
 * Item (e, j) is the segment a -> b, a = the xyz of `from` (e, j), b = the xyz of `to` (e, j), fp32 taken to fp64; the swept solid
 * is the sphere of radius R = (double)radius moved along it (a capsule).  The body turns in flight, so the
 * orientation-independent solid is the sphere that bounds the cylinder, R = sqrt(radius^2 + half_length^2) of
 * gnbv_collide_cylinder's body: conservative, it never passes a path the cylinder could not fly.  The code of item (e, j) is
 *   8  (PATH):        some closed triangle T of env e has dist(segment, T) <= R (a degenerate triangle counts as its segment or
 *                     point; a zero-length segment is the sphere test), OR
 *   16 (PATH_GROUND): ground != 0 and min(a_z, b_z) - R <= 0.
 * The bits coexist with gnbv_collide_cylinder's 1, 2 and 4 in one byte.  An item with a non-finite endpoint gets 0.  There is
 * no "inside" bit: a path whose start is free cannot enter a closed solid without coming within R of one of its triangles;
 * whether the start is free is gnbv_collide_cylinder's question.
 * to [N, K, >= 3] with the stride between consecutive (e, j) rows in floats (>= 3); from: row (e, j) at
 * from + e * from_env_stride + j * from_item_stride floats, from_env_stride >= 3, from_item_stride >= 3 or 0 = one start per env,
 * broadcast over K.  episode_length [N] int64 or NULL: where episode_length[e] <= 1 the code of every item of env e is 0 -- the
 * first pose of an episode is set, not flown to (the tensor gnbv_env_pre_step counts).  accumulate = 0 stores the code,
 * 1 ORs it into contact_out[e, j] (the item's own wave reads and writes its own byte: no atomics), e.g. onto what
 * gnbv_collide_cylinder_batch has just stored.  Deterministic; no host synchronisation, no allocation, no workspace.
 * k >= 1, N * k <= 2^31 - 1, radius > 0 finite, accumulate 0 or 1, else hipErrorInvalidValue. */
int gnbv_sweep_sphere(const GnbvMeshScene *scene /*[host]*/, const float *from, int64_t from_env_stride /*floats*/,
                      int64_t from_item_stride /*floats, 0 = broadcast*/, const float *to, int k, int64_t to_row_stride /*floats*/,
                      float radius, int ground, const int64_t *episode_length /*[N] or NULL*/, int accumulate,
                      uint8_t *contact_out /*[N,K]*/, void *stream);

/* Collision-free flight between views (new entry points of ABI 5): the shortest 26-connected route over the flight lattice.
 * The lattice has nx * ny * nz = M nodes (each axis 1..1024), node (i, j, k) at lo + h * (i, j, k), flat id c = (k ny + j) nx + i,
 * the same for every env (gennbv_amd/env/flight.py).  blocked [N, ceil(M / 32)] u32: bit c & 31 of word c >> 5 of env e is set
 * where node c is not free in env e (MeshScene.flight_blocked; padding bits are not read).  Two free nodes that differ by at
 * most one step on every axis are joined by an edge of cost[|dx| | |dy| << 1 | |dz| << 2] millimetres ([host], 8 u32, every
 * entry the lattice can use > 0, M * max cost < 2^32 - 2): all distances are integer sums, so the result is exact and does not
 * depend on the order of evaluation.  The nearest node of a pose is, per axis, clamp(floor((p - lo) / h + 0.5), 0, n - 1) in
 * fp64 (0 on an axis with one node); a pose with a non-finite x, y or z has no node.  lo, h [host] 3 doubles, finite, h > 0 on
 * every axis with more than one node.  No allocation, no host synchronisation; bad arguments return hipErrorInvalidValue. */

/* The most nodes whose field fits the LDS of one CU (mode 1 of gnbv_flight_field): (160 KiB - 16) / 4 = 40956. */
int gnbv_flight_lds_max_nodes(void);
/* field_out[e, c] = the length in mm of the shortest route from the nearest node of poses[e] (row stride in floats, >= 3) to
 * node c through free nodes; the source holds 0; blocked and unreachable nodes hold 0xFFFFFFFF, and so does every node of an env
 * whose source node is blocked or absent.  One workgroup per env relaxes the table in place until a sweep changes nothing.
 * mode: 0 auto (1 where M <= gnbv_flight_lds_max_nodes(), else 2), 1 the table resident in LDS (hipErrorInvalidValue where it does
 * not fit), 2 the table in field_out itself; the result is the same.  status_out[e] = 0, or 1 where the sweep count reached its
 * hard cap M before the table settled (it cannot: Bellman-Ford needs fewer than M sweeps; the cap bounds the loop whatever
 * happens, and the field of such an env is not to be used). */
int gnbv_flight_field(const uint32_t *blocked /*[N,ceil(M/32)]*/, int n, int nx, int ny, int nz, const uint32_t *cost /*[host] 8*/,
                      const float *poses, int64_t poses_row_stride /*floats*/, const double *lo /*[host] 3*/,
                      const double *h /*[host] 3*/, uint32_t *field_out /*[N,M]*/, int32_t *status_out /*[N]*/, int mode, void *stream);
/* cost_mm_out[e, j] = field[e, nearest node of targets (e, j)], 0xFFFFFFFF for a target without a node.  targets [N, K, >= 3] with
 * the stride between consecutive (e, j) rows in floats (>= 3); k >= 1, N * k <= 2^31 - 1. */
int gnbv_flight_query(const uint32_t *field /*[N,M]*/, int n, int nx, int ny, int nz, const double *lo /*[host] 3*/,
                      const double *h /*[host] 3*/, const float *targets, int k, int64_t targets_row_stride /*floats*/,
                      uint32_t *cost_mm_out /*[N,K]*/, void *stream);
/* The route of one target per env (targets [N, >= 3], row stride in floats), as node ids from the target's nearest node back
 * to the source: from each node the walk takes the first neighbour, in the fixed order dz, dy, dx in (-1, 0, 1) with dx
 * fastest, with field[neighbour] + cost == field[node].  len_out[e] = the number of nodes (1 when target and source share a
 * node), 0 for an unreachable target, and -needed where the route has more than max_len nodes (the first max_len are
 * written).  nodes_out [N, max_len], max_len >= 1. */
int gnbv_flight_path(const uint32_t *field /*[N,M]*/, int n, int nx, int ny, int nz, const uint32_t *cost /*[host] 8*/,
                     const double *lo /*[host] 3*/, const double *h /*[host] 3*/, const float *targets,
                     int64_t targets_row_stride /*floats*/, int32_t *nodes_out /*[N,max_len]*/, int max_len, int32_t *len_out /*[N]*/,
                     void *stream);

/* Unknown space at a price (additive entry points of ABI 5): gnbv_flight_field / gnbv_flight_path with a penalty for entering a
 * "costly" node.  costly [N, ceil(M / 32)] u32, the layout of `blocked`; a costly bit on a blocked node is ignored, padding bits are
 * not read.  field_out[e, c] = the minimum, over routes from the source node to c through non-blocked nodes, of the sum of the edge
 * costs plus penalty_mm times the number of costly nodes entered on the route (c included, the source not); the source holds 0,
 * blocked and unreachable nodes 0xFFFFFFFF, and so does every node of an env whose source is blocked or absent.  Integer sums: the
 * result is exact and independent of the order of relaxation; with penalty_mm = 0 or an all-zero `costly` it is byte for byte
 * gnbv_flight_field's.  Modes, status_out and the sweep cap as gnbv_flight_field.  Refused (hipErrorInvalidValue, before any launch)
 * for everything gnbv_flight_field refuses, a NULL costly, and M * (max used cost + penalty_mm) >= 0xFFFFFFFE (in 64 bits). */
int gnbv_flight_field_w(const uint32_t *blocked /*[N,ceil(M/32)]*/, const uint32_t *costly /*[N,ceil(M/32)]*/, uint32_t penalty_mm, int n,
                        int nx, int ny, int nz, const uint32_t *cost /*[host] 8*/, const float *poses, int64_t poses_row_stride /*floats*/,
                        const double *lo /*[host] 3*/, const double *h /*[host] 3*/, uint32_t *field_out /*[N,M]*/,
                        int32_t *status_out /*[N]*/, int mode, void *stream);
/* gnbv_flight_path over a field of gnbv_flight_field_w (the same costly and penalty_mm): from each node the walk takes the first
 * neighbour, in the fixed order dz, dy, dx with dx fastest, with field[neighbour] < field[node] and
 * field[neighbour] + cost + penalty_mm * costly(node) == field[node].  len_out as gnbv_flight_path.  gnbv_flight_query reads such a
 * field unchanged. */
int gnbv_flight_path_w(const uint32_t *field /*[N,M]*/, const uint32_t *costly /*[N,ceil(M/32)]*/, uint32_t penalty_mm, int n, int nx,
                       int ny, int nz, const uint32_t *cost /*[host] 8*/, const double *lo /*[host] 3*/, const double *h /*[host] 3*/,
                       const float *targets, int64_t targets_row_stride /*floats*/, int32_t *nodes_out /*[N,max_len]*/, int max_len,
                       int32_t *len_out /*[N]*/, void *stream);

/* The free set of the flight lattice from the scanned map (an additive entry point of ABI 5; csrc/flightmap.hip): the blocked bits
 * gnbv_flight_field reads, from each env's tri-class grid instead of the ground-truth mesh.  tri [G,G,G] per env in C order x, y, z
 * with gnbv_view_gain's signs: < 0 free, 0 unknown, > 0 occupied.  Exactly one of the two forms: tri_i8 (int8 rows, row stride in
 * bytes) or tri_f32 (fp32 rows, row stride in floats: the grid slice of a flat observation row); the other NULL.  range_gt [N,6],
 * voxel_size [N,3] device arrays; the lattice as above (lo, h [host] 3 doubles); rho [host] the radius of the ball round a node.
 * The predicate, in fp64, in this operation order, without FMA:
 *   voxel frame (gnbv_pose_to_idx): v_a = (double)voxel_size[a], o_a = (double)fp32(range_gt[2a+1] - fp32(0.5f * voxel_size[a]));
 *     voxel i of axis a spans [o_a + i v_a, o_a + (i + 1) v_a]; node c sits at p_a = lo_a + h_a * idx_a.
 *   window per axis: i0_a = floor(((p_a - rho) - o_a) / v_a), i1_a = floor(((p_a + rho) - o_a) / v_a), both clamped in fp64 to
 *     [0, G - 1] before conversion; the window is empty if i1_a < 0 or i0_a > G - 1 (before clamping) on any axis.
 *   a voxel of the window is touched iff (gx^2 + gy^2) + gz^2 <= rho * rho,
 *     g_a = max(max((o_a + i v_a) - p_a, 0), p_a - (o_a + (i + 1) v_a)).
 *   the node touches the outside iff on any axis p_a - rho < o_a or p_a + rho > o_a + (double)G * v_a.
 * Bit c of env e is set iff a touched voxel is occupied, or unknown_blocks and a touched voxel is unknown, or outside_blocks and
 * the node touches the outside, or ground and p_z - rho <= 0.  blocked_out [N, ceil(M / 32)], every word written, padding bits set.
 * mode: 0 auto (1 where G <= gnbv_flightmap_lds_max_grid(), else 2), 1 one bit per voxel packed into LDS first
 * (hipErrorInvalidValue where G^3 / 8 bytes do not fit), 2 the grid read from global memory; the result is the same.  One launch,
 * one writer per output word, no atomics, no allocation, no host synchronisation; every loop is bounded by G whatever the device
 * arrays hold.  hipErrorInvalidValue before any launch for: both or neither grid form, a NULL required pointer, n < 1, G outside
 * 1..128, a row stride below G^3, rho not finite or <= 0, a lattice axis outside 1..1024 or lo / h not finite (h > 0 where the
 * axis has more than one node), a mode outside 0..2. */
int gnbv_flightmap_lds_max_grid(void); /* the largest G of mode 1: 109 */
int gnbv_flight_blocked_tri(const int8_t *tri_i8 /*[N, >= G^3] or NULL*/, int64_t tri_i8_row_stride /*bytes*/,
                            const float *tri_f32 /*[N, >= G^3] or NULL*/, int64_t tri_f32_row_stride /*floats*/, int g,
                            const float *range_gt /*[N,6]*/, const float *voxel_size /*[N,3]*/, int n, int nx, int ny, int nz,
                            const double *lo /*[host] 3*/, const double *h /*[host] 3*/, double rho, int unknown_blocks,
                            int outside_blocks, int ground, uint32_t *blocked_out /*[N,ceil(M/32)]*/, int mode, void *stream);

/* gnbv_flight_blocked_tri with unknown space told apart, in one launch (an additive entry point of ABI 5): the arguments of
 * gnbv_flight_blocked_tri without unknown_blocks, two outputs [N, ceil(M / 32)], every word of both written.  The predicate, the
 * voxel frame and the rule of the window are those above.  blocked_out = gnbv_flight_blocked_tri(unknown_blocks = 0, the same
 * outside_blocks and ground), padding bits set.  Bit c of costly_out is set iff node c is not blocked and a touched voxel is
 * unknown -- gnbv_flight_blocked_tri(unknown_blocks = 1) & ~blocked_out inside M -- padding bits clear.  mode 1 packs two bit planes
 * (occupied, unknown) into LDS and is refused above gnbv_flightmap_classify_lds_max_grid(); the other refusals, the loop bounds and
 * "one launch, one writer per word, no atomics, no workspace, no host synchronisation" as gnbv_flight_blocked_tri; a NULL costly_out
 * is refused too. */
int gnbv_flightmap_classify_lds_max_grid(void); /* the largest G of mode 1 of gnbv_flight_classify_tri: 86 */
int gnbv_flight_classify_tri(const int8_t *tri_i8 /*[N, >= G^3] or NULL*/, int64_t tri_i8_row_stride /*bytes*/,
                             const float *tri_f32 /*[N, >= G^3] or NULL*/, int64_t tri_f32_row_stride /*floats*/, int g,
                             const float *range_gt /*[N,6]*/, const float *voxel_size /*[N,3]*/, int n, int nx, int ny, int nz,
                             const double *lo /*[host] 3*/, const double *h /*[host] 3*/, double rho, int outside_blocks, int ground,
                             uint32_t *blocked_out /*[N,ceil(M/32)]*/, uint32_t *costly_out /*[N,ceil(M/32)]*/, int mode, void *stream);

/* A straight flight judged on the scanned map (an additive entry point of ABI 5; csrc/sweepmap.hip): the sphere of radius R moved
 * along N x K straight legs against each env's tri-class grid.  The grid forms, the signs (< 0 free, 0 unknown, > 0 occupied), the
 * voxel order (x G + y) G + z and the voxel frame (o_a, v_a; voxel i of axis a spans [o_a + i v_a, o_a + (i + 1) v_a]) are those of
 * gnbv_flight_blocked_tri; the item layout (from / to, the strides, xyz the first three floats of a row) is gnbv_sweep_sphere's.
 * Item (e, j) is the segment a -> b, fp32 taken to fp64, x(s) = a + s (b - a).  code_out[e, j], one byte:
 *   1 (MAP):     some voxel that is occupied, or unknown with unknown_blocks, is touched:
 *                min over s in [0, 1] of sum_a g_a(s)^2 <= R^2, g_a(s) = max(lo_a - x_a(s), 0, x_a(s) - hi_a) -- the distance from the
 *                segment to the closed box, evaluated in closed form in fp64 (the ends, the at most six breakpoints where a
 *                coordinate crosses a face, each piece's vertex clamped to the piece).  A zero-length segment gives the ball test
 *                of gnbv_flight_blocked_tri.
 *   2 (OUTSIDE): outside_blocks and, on some axis, min(a_a, b_a) - R < o_a or max(a_a, b_a) + R > o_a + (double)G v_a.
 *   4 (GROUND):  ground and min(a_z, b_z) - R <= 0.
 * An item with a non-finite coordinate gets 0.  mode: 0 auto (1 where G <= gnbv_sweepmap_lds_max_grid(), else 2), 1 one bit per
 * voxel packed into LDS per workgroup (hipErrorInvalidValue where the bits do not fit), 2 the grid read from global memory; the
 * result is the same.  One launch, one writer per byte, no atomics, no workspace, no allocation, no host synchronisation; every
 * loop is bounded by a function of G and compile-time constants whatever the device arrays hold.  hipErrorInvalidValue before any
 * launch for: both or neither grid form, a NULL required pointer, n < 1, k < 1, N * k > 2^31 - 1, G outside 1..128, a grid row
 * stride below G^3, to_row_stride or from_env_stride < 3, from_item_stride neither 0 nor >= 3, radius not finite or <= 0, a mode
 * outside 0..2, mode 1 above its limit. */
int gnbv_sweepmap_lds_max_grid(void); /* the largest G of mode 1: 109 */
int gnbv_sweep_tri(const int8_t *tri_i8 /*[N, >= G^3] or NULL*/, int64_t tri_i8_row_stride /*bytes*/,
                   const float *tri_f32 /*[N, >= G^3] or NULL*/, int64_t tri_f32_row_stride /*floats*/, int g,
                   const float *range_gt /*[N,6]*/, const float *voxel_size /*[N,3]*/, int n, const float *from,
                   int64_t from_env_stride /*floats*/, int64_t from_item_stride /*floats, 0 = broadcast*/, const float *to, int k,
                   int64_t to_row_stride /*floats*/, double radius, int unknown_blocks, int outside_blocks, int ground,
                   uint8_t *code_out /*[N,K]*/, int mode, void *stream);

/* The frontier of the scanned map (an additive entry point of ABI 5; csrc/frontier.hip): the boundary between what each env's
 * tri-class grid knows to be free and what it does not know.  The grid forms (exactly one of tri_i8 / tri_f32, row stride in bytes /
 * floats), the signs (< 0 free, 0 unknown, > 0 occupied) and the voxel order (x G + y) G + z are those of gnbv_flight_blocked_tri.
 * Voxel (x, y, z) of env e is a frontier voxel iff its class is unknown and at least one of its six face neighbours that lie inside
 * the grid is free; a neighbour outside the grid is no neighbour (the voxel that follows (x, y, G - 1) in memory is not its
 * z-neighbour).  Integers only: one right answer.
 *   bits_out   [N, ceil(G^3 / 32)] u32 or NULL: bit vox & 31 of word vox >> 5, unswizzled; every word written, padding bits clear.
 *   blocks_out [N, nb^3, 4] int32, nb = ceil(G / block): the record of block (bx nb + by) nb + bz covers the voxels with
 *              x / block == bx, y / block == by, z / block == bz and holds {count, sum x, sum y, sum z} over its frontier voxels;
 *              every record written, zeros where empty.  The frontier count of an env is the sum of its records' counts.
 * One launch over workgroups (env, slab of x-planes); `slab` is the slab height in planes, 0 = auto; a given height is rounded up
 * to a multiple of `block` and lowered to what the two LDS bit planes admit ((slab + 2) G^2 / 4 bytes).  The result is the same for
 * every slab.  One writer per output word and per record, no atomics, no workspace, no allocation, no host synchronisation; every
 * loop is bounded by a function of G and compile-time constants whatever the device arrays hold.  hipErrorInvalidValue before any
 * launch for: both or neither grid form, a NULL blocks_out, n < 1, G outside 1..128, block outside 1..16, a row stride below G^3,
 * slab < 0. */
int gnbv_frontier_tri(const int8_t *tri_i8 /*[N, >= G^3] or NULL*/, int64_t tri_i8_row_stride /*bytes*/,
                      const float *tri_f32 /*[N, >= G^3] or NULL*/, int64_t tri_f32_row_stride /*floats*/, int g, int n, int block,
                      uint32_t *bits_out /*[N,ceil(G^3/32)] or NULL*/, int32_t *blocks_out /*[N,nb^3,4]*/, int slab /*0 = auto*/,
                      void *stream);

/* Frontier viewpoints (an additive entry point of ABI 5; csrc/frontview.hip): for T target voxels per env, which node of the flight
 * lattice sees the target on the scanned map, and which of those is cheapest to fly to.  The grid forms (exactly one of tri_i8 /
 * tri_f32, row stride in bytes / floats), the signs (< 0 free, 0 unknown, > 0 occupied), the voxel order (x G + y) G + z and the
 * voxel frame are those of gnbv_flight_blocked_tri; the lattice (nx, ny, nz, lo, h; node c = (k ny + j) nx + i) and `field` [N, M]
 * u32 (0xFFFFFFFF = no route; any table in that layout) are those of gnbv_flight_field / _w; the ray rule is gnbv_view_gain's.
 * Integers and fp64 in a stated order: one right answer.  For env e and target j = (tx, ty, tz) of targets [N, T, 3] int32:
 *   voxel frame: v_a = (double)voxel_size[a], o_a = (double)fp32(range_gt[2a+1] - fp32(0.5f * voxel_size[a])); the target point is
 *     q_a = o_a + ((double)t_a + 0.5) * v_a.  A target with any coordinate outside [0, G) is NO TARGET.
 *   distance: node c sits at p_a = lo_a + h_a * idx_a (fp64); d2 = ((p_x - q_x)^2 + (p_y - q_y)^2) + (p_z - q_z)^2 in this
 *     operation order, without FMA; the node is IN RANGE iff r_min * r_min <= d2 <= r_max * r_max.
 *   line of sight: the source voxel is gnbv_pose_to_idx((float)p_x, (float)p_y, (float)p_z), unclamped (voxel coordinates beyond
 *     +-2^24 saturate there); the line is gnbv_bresenham3d's from the source to the target (not symmetric: source first); its
 *     in-grid voxels in order are w_0 .. w_L, w_L the target.  The node SEES the target iff none of w_0 .. w_{L-1} is occupied and
 *     at most max_unknown of them are unknown.  The class of the target voxel itself is not looked at; L = 0 sees it.
 *   node_out  [N,T] int32:   among the nodes in range that see the target and have field[e, c] != 0xFFFFFFFF, the one with the
 *                            smallest (field[e, c], c) in lexicographic order; -1 where there is none, or no target.
 *   cost_out  [N,T] u32:     its field value; 0xFFFFFFFF where node_out is -1.
 *   count_out [N,T,2] int32: {nodes in range that see the target, of which with a route}.
 * Every element of the three outputs is written.  The result is defined over all M nodes; the kernel visits the index window
 * round the target that |p_a - q_a| <= r_max admits, one node wider on both sides and wider still by 2^-48 of the magnitudes
 * involved over h_a (the rounding of p_a and of the window's own arithmetic), clamped to the lattice in fp64.
 * mode: 0 auto (2 at every G: measured faster than 1 at every size tried), 1 the grid's classes packed into two LDS bit planes per
 * workgroup (hipErrorInvalidValue where G > gnbv_frontview_lds_max_grid()), 2 the grid read in place; the result is the same.  chunk: targets per
 * workgroup, 0 = chosen from n and t; any value gives the same result.  One launch, one writer per output element, no global
 * atomics, no workspace, no allocation, no host synchronisation; every loop is bounded by a function of G, the lattice dimensions
 * and compile-time constants whatever field, targets and the grid hold.  hipErrorInvalidValue before any launch for: both or
 * neither grid form, a NULL required pointer, n < 1, t < 1, N * T > 2^31 - 1, G outside 1..128, a row stride below G^3, a lattice
 * axis outside 1..1024, lo / h not finite or h <= 0 on an axis with more than one node, r_min / r_max not finite, r_min < 0,
 * r_max <= 0, r_min > r_max, max_unknown < 0, chunk < 0, a mode outside 0..2, mode 1 above its limit.
 * [host struct]; pointers are device unless noted. */
typedef struct GnbvFrontView {
    int n, t, g;                    /* envs, targets per env, grid edge */
    const int8_t *tri_i8;           /* [n, >= g^3] or NULL; row stride in bytes */
    int64_t tri_i8_row_stride;
    const float *tri_f32;           /* [n, >= g^3] or NULL; row stride in floats */
    int64_t tri_f32_row_stride;
    const float *range_gt;          /* [n, 6] */
    const float *voxel_size;        /* [n, 3] */
    int nx, ny, nz;                 /* the flight lattice */
    double lo[3], h[3];
    const uint32_t *field;          /* [n, nx ny nz] */
    const int32_t *targets;         /* [n, t, 3] voxel coordinates */
    double r_min, r_max;            /* metres */
    int max_unknown;
    int32_t *node_out;              /* [n, t] */
    uint32_t *cost_out;             /* [n, t] */
    int32_t *count_out;             /* [n, t, 2] */
    int chunk;                      /* targets per workgroup, 0 = auto */
    int mode;                       /* 0 auto, 1 LDS bit planes, 2 the grid in place */
} GnbvFrontView;
int gnbv_frontview_lds_max_grid(void); /* the largest G of mode 1: 86 */
int gnbv_frontier_viewpoints(const GnbvFrontView *args /*[host]*/, void *stream);

/* compute_reward (env_train_base.py:377-398), _reward_* / check_termination /
 * reset_idx (env_train_gennbv.py:377-457,535-556), update_extra_episode_info
 * (env_train_base.py:629-639). All pointers device, arrays [N] unless noted. [host struct] */
typedef struct GnbvEnvPost {
    int n;
    int only_positive;              /* cfg.rewards.only_positive_rewards */
    int64_t max_episode_length;
    float scale_cov, scale_short, scale_term; /* reward scales * dt, rounded to fp32 */
    float coverage_threshold;       /* 0.99 */
    const int32_t *coverage_count;  /* from gnbv_update_occ_grid */
    const float *num_valid_voxel_gt;
    float *prev_ratio;              /* in/out: reward_ratio_buf[-1] */
    int64_t *episode_length_buf;    /* in/out */
    float *rewards;                 /* out */
    uint8_t *dones;                 /* out: reset_buf */
    uint8_t *reset_mask;            /* out: envs whose grids/history reset before the next step */
    uint8_t *step_time_out;         /* out: time_out_buf of this step */
    uint8_t *extras_time_outs;      /* in/out: infos["time_outs"] (refreshed only if any env reset) */
    float *coverage_ratio;          /* out */
    float *episode_sums;            /* in/out [3,N]: surface_coverage, short_path, termination */
    float *cur_reward_sum;          /* in/out */
    float *cur_episode_length;      /* in/out */
    float *ring_reward;             /* in/out [ring_len]: rewbuffer (deque maxlen 100) */
    float *ring_length;             /* in/out [ring_len]: lenbuffer */
    int64_t *ring_state;            /* in/out [1]: episodes finished so far */
    int ring_len;
    double *episode_info;           /* out [6] or NULL: extras["episode"] as it stands after THIS step, fp64:
                                       [0] generation = number of dict objects the reference has created so far (a new
                                           one on every step where some env resets, env_train_gennbv.py:424; steps in
                                           between mutate and re-emit the SAME dict, so earlier buffer entries alias it),
                                       [1] episode_reward, [2] episode_length = np.mean of the rewbuffer / lenbuffer
                                           deques (env_train_base.py:638-639; 0 when empty),
                                       [3..5] rew_<name> = mean(episode_sums[name][reset envs]) / max_episode_length_s
                                           of the dict's creation step (:425-427) */
    double *episode_state;          /* in/out [4], required with episode_info: generation, rew_<name> x 3 */
    float max_episode_length_s;     /* cfg.env.episode_length_s */
} GnbvEnvPost;

int gnbv_env_post_step(const GnbvEnvPost *args /*[host]*/, void *stream);
/* The same with collision termination (a new entry point of ABI 5, no layout changes): check_termination's collision_buf
 * (env_train_gennbv.py:438-457) is contact [N] u8 (gnbv_collide_cylinder's code; != 0 = collided), and an env resets when
 * contact[e] != 0 || time_out || coverage ratio > threshold.  A collision is a reset that is not a time-out: it earns the
 * termination reward, and its episode sums, ring-buffer entries and episode_info behave as on any other reset.
 * contact == NULL: exactly gnbv_env_post_step. */
int gnbv_env_post_step_contacts(const GnbvEnvPost *args /*[host]*/, const uint8_t *contact /*[N] or NULL*/, void *stream);

/* Tail of one rollout step in one launch: the time-out bootstrap `rewards += gamma * squeeze(terminal_value * time_outs)`
 * (on_policy_algorithm_grid_obs.py:205-208; same fp32 operation order; terminal_value_stride = 1: env i uses
 * terminal_value[i]; 0: every env uses terminal_value[0] -- what the reference computes, its `predict_values(new_obs)[0]`
 * takes ROW 0 of the [N,1] values and broadcasts it over the envs) and the five copies of
 * TensorRolloutBuffer_Grid_Obs.add (stable_baselines3/common/buffers.py:676-704) into row `step` of the buffer arrays
 * (caller passes the row pointers): actions int64 [N,A] -> f32, episode_starts bool/u8 [N] -> u8, rewards / values /
 * log_probs f32 [N].  time_outs: bool/u8 [N]. */
int gnbv_rollout_add(int n, int action_dim, const int64_t *actions, const float *rewards, const uint8_t *time_outs,
                     const float *terminal_value, int terminal_value_stride, float gamma, const uint8_t *episode_starts,
                     const float *values, const float *log_probs, float *buf_actions, float *buf_rewards, uint8_t *buf_episode_starts,
                     float *buf_values, float *buf_log_probs, void *stream);

/* ------------------------------------------------------------------------- */
/* B1  Hybrid_Encoder grid branch (gennbv/network/hybrid_encoder.py:38-45,90-94): */
/*     Conv3d(1,16,3,s2) BN ReLU Conv3d(16,16,3,s2) BN ReLU -> flatten             */
/*     fp32, forward + backward, hand-written MFMA kernels (csrc/encoder.hip).     */
/* ------------------------------------------------------------------------- */
/* Device pointers to the parameters / buffers of `naive_encoder_grid`
 * (torch layouts: w1 [16,1,3,3,3], w2 [16,16,3,3,3], vectors [16]). [host struct] */
typedef struct GnbvEncoderParams {
    const float *w1, *b1, *bn1_w, *bn1_b;
    float *bn1_rm, *bn1_rv;       /* running_mean / running_var (updated when training) */
    int64_t *bn1_nbt;             /* num_batches_tracked [1] or NULL */
    const float *w2, *b2, *bn2_w, *bn2_b;
    float *bn2_rm, *bn2_rv;
    int64_t *bn2_nbt;
    float eps, momentum;          /* 1e-5, 0.1 (torch.nn.BatchNorm3d defaults) */
    const int8_t *grid_i8;        /* NULL, or an int8 copy of the grid slices (values -1/0/1, as written by
                                     gnbv_update_occ_grid_coded): sample b reads grid_i8 + (rows ? rows[b] : b) *
                                     grid_i8_row_stride bytes instead of obs_grid (a quarter of the input traffic);
                                     used by the LDS-staged kernels when grid % 16 == 0, otherwise obs_grid is read --
                                     unless obs_grid == NULL (compact observations: the grid exists only as these
                                     rows; any grid size, fp32 activations) */
    int64_t grid_i8_row_stride;
    const int32_t *autocorr;      /* NULL, or per-sample input autocorrelation rows (gnbv_input_autocorr over the same
                                     int8 rows, same row numbering): the fused backward sums rows[b]'s rows instead of
                                     recomputing the minibatch's autocorrelation */
    int64_t autocorr_row_stride;  /* ints */
    /* ---- data-parallel replicas: BatchNorm over the GLOBAL minibatch.  world <= 1 / sync_sum == NULL: a single
     * replica, nothing below is read.  Otherwise the training forward / backward call sync_sum three times -- BN2 batch sums
     * (forward), BN2-backward sums and BN1-backward sums (backward) -- each time on 32 doubles of `sync_buf`, and the
     * statistics of BatchNorm-1 come from `autocorr_global`.  Needs the fused backward (aligned int8 rows + autocorr rows). */
    int world;                    /* number of replicas */
    int (*sync_sum)(void *ctx, int offset, int n, void *stream);  /* [host callback] sum sync_buf[offset, offset + n) over the
                                     replicas in place, ordered on `stream` (e.g. an all-reduce enqueued there); returns 0 */
    void *sync_ctx;
    double *sync_buf;             /* device [96] */
    const int32_t *autocorr_global; /* device [768]: sum of the autocorrelation rows of ALL replicas' minibatch rows */
    /* ---- operand ranges of the split-f16 kernels (ABI 2).  At G = 64 the conv stack runs on the f16 matrix pipe with every
     * fp32 operand written as hi + lo f16 halves under fixed power-of-two scalings: relu(bn1(y1)) <= 253.9, |W2| < 63,
     * fc_grid inputs <= 1015, |W_fc| < 15.8.  Outside those ranges the split kernels would clamp, so: */
    const int32_t *autocorr_total;/* NULL, or device [768]: the SUM of the minibatch's autocorrelation rows, computed by the caller (the
                                     permutation is fixed for a whole train() call: one table for all its minibatches) -- the training
                                     forward then skips its gather of `autocorr` rows (128 scattered 3 KiB rows, ~6 us of dependent
                                     round trips on the update's critical path); `autocorr` must still be set (it selects the path) */
    int force_fp32;               /* 1: never take the split-f16 kernels (the fp32-MFMA kernels have no range limits); the host
                                     mirror sets it when a parameter pre-check finds a weight outside its range */
    int32_t *range_flag;          /* NULL, or a device word the kernels OR bits into when an ACTIVATION bound is reached:
                                     2 = a BatchNorm-1 channel whose parameter bound |scale| sum|W1| + |scale b1 + shift| exceeds
                                     253 (conv1's input is tri-class, |x| <= 1); 4 = a feature (fc_grid input) above 1000.
                                     The caller reads it once per train() / rollout; a non-zero word means the results of the
                                     calls since the last check may be clamped: raise, or repeat with force_fp32 */
    int eval_prepared;            /* (ABI 5) inference only (training == 0), 0 by default.  1: the caller ran gnbv_encoder_eval_prepare()
                                     for THESE parameters, this (batch, grid), this `bn_state` and this `workspace` since the parameters
                                     or BatchNorm's running statistics last changed, and nothing else has written bn_state / used the
                                     workspace since: the forward then skips the launches that only depend on the parameters
                                     (BatchNorm scale / shift of both layers, the conv2 weight images) -- three small kernels on the
                                     critical path of every env step of a rollout (sb3/ppo_grid_obs.py collect_rollouts: the
                                     parameters are fixed between two train() calls).  Ignored where the inference path has no
                                     such launches to skip. */
} GnbvEncoderParams;

typedef struct GnbvEncoderGrads {  /* outputs, same shapes as the parameters */
    float *w1, *b1, *bn1_w, *bn1_b, *w2, *b2, *bn2_w, *bn2_b;
} GnbvEncoderGrads;

/* Input autocorrelation of the conv1 patches of n int8 grid rows (values -1/0/1): out row e (gnbv_input_autocorr_row_ints()
 * = 768 ints: the 16x16 tiles [0..15][0..15], [0..15][16..31], [16..31][16..31] of the symmetric R[32][32]) holds
 * R[t][t'] = sum over the O1^3 conv1 output positions of x[pos, t] * x[pos, t'], t = 0..26 the taps of
 * hybrid_encoder.py:39's Conv3d(1, 16, k3, s2), t = 27 a constant 1 (R[t][27] = sum x, R[27][27] = O1^3).  Exact (int8
 * MFMA).  BatchNorm-backward of that layer is linear in the input, so these rows replace every reduction over the
 * layer's activations that does not involve the incoming gradient (encoder.hip, k_conv2_dgrad_c1w).  G % 16 == 0,
 * 3 G^2 <= 64 KiB. */
int gnbv_input_autocorr_row_ints(void);
int gnbv_input_autocorr(const int8_t *grid_i8, int64_t grid_i8_row_stride, int n, int grid, int32_t *out, int64_t out_row_stride,
                        void *stream);

size_t gnbv_encoder_workspace_bytes(int batch, int grid);
/* The parameter-only part of an INFERENCE forward (see GnbvEncoderParams.eval_prepared): BatchNorm-1 / -2 scale, shift, mean, rstd
 * from the running statistics into bn_state, the conv2 weight images into the workspace.  Returns 0 when done, and
 * GNBV_ERR_NOT_APPLICABLE (-2) -- nothing launched, nothing to skip -- where the inference forward of this (params, grid) does
 * not take the one-launch conv1 + conv2 kernel (then call gnbv_encoder_grid_forward with eval_prepared = 0 as before). */
#define GNBV_ERR_NOT_APPLICABLE (-2)
int gnbv_encoder_eval_prepare(int batch, int grid, const GnbvEncoderParams *params, float *bn_state, void *workspace, size_t workspace_bytes,
                              void *stream);
/* number of fp32 ELEMENTS of the layer-1 activation buffers (y1, dz1_scratch) */
size_t gnbv_encoder_y1_elems(int batch, int grid);

/* obs_grid: pointer to the grid slice of row 0 of an observation matrix (NULL with params->grid_i8 set: compact
 * observations); sample b reads
 * obs_grid + (rows ? rows[b] : b) * row_stride floats (the minibatch gather of
 * buffers.py:753-762 is fused into the read).  training != 0: BatchNorm uses batch statistics
 * and updates the running stats (unless *skip_flag != 0), else the running stats.
 * Saved for backward: y1 (gnbv_encoder_y1_elems floats: channels-last, x-parity-split, pre-BN),
 * y2 [B,16,O2^3] (pre-BN),
 * bn_state: 128 floats [2][4][16] (scale, shift, mean, rstd per layer) + 768 ints (the minibatch total of the input
 * autocorrelation, written when the forward derived BatchNorm-1's statistics from it and read back by the backward):
 * 896 four-byte words.
 * features [B, 16*O2^3] is the reference's `naive_encoder_grid(x).reshape(num_env, -1)`; NULL: not written (the BatchNorm-2 + ReLU pass is
 * left to gnbv_linear_forward_fold / gnbv_linear_bwd_dw_fold, which form the activations from y2 and bn_state in registers). */
int gnbv_encoder_grid_forward(const float *obs_grid, const int64_t *rows, int64_t row_stride, int batch, int grid,
                              const GnbvEncoderParams *params /*[host]*/, int training, const int *skip_flag, void *y1,
                              float *y2, float *bn_state, float *features, void *workspace, size_t workspace_bytes,
                              void *stream);

/* Gradients of all eight parameter tensors given d_features [B, 16*O2^3].  Must follow a gnbv_encoder_grid_forward call
 * with training != 0 and the same obs / rows / params arguments (it consumes that call's y1, y2 and bn_state, including the
 * autocorrelation total when the forward left one there).
 * dy2_scratch [B,O2^3,16] and dz1_scratch (gnbv_encoder_y1_elems floats) are caller-owned scratch. */
int gnbv_encoder_grid_backward(const float *obs_grid, const int64_t *rows, int64_t row_stride, int batch, int grid,
                               const GnbvEncoderParams *params /*[host]*/, const void *y1, const float *y2,
                               const float *bn_state, const float *d_features, float *dy2_scratch, void *dz1_scratch,
                               const GnbvEncoderGrads *grads /*[host]*/, void *workspace, size_t workspace_bytes,
                               void *stream);

/* B1  Hybrid_Encoder.output_layer_grid = Linear(16*o2^3, 256) + ReLU
 *     (gennbv/network/hybrid_encoder.py:39-42, applied at :87).  out[m][n] = act(bias[n] + sum_k x[m][k] w[n][k]),
 *     x [M][K], w [N][K] (torch.nn.Linear.weight layout), K % 4 == 0, N % 64 == 0, all pointers 16-byte aligned.
 *     Deterministic split-K (fixed summation order).  `relu` is a flag word: bit 0 fuses the ReLU; bit 1 forces the fp32-MFMA
 *     kernel (no operand-range limits) where the default is the split-f16 kernel, which CLAMPS |x| at 1015 and |w| at 15.8
 *     (the caller checks its ranges: GnbvEncoderParams.range_flag bit 4 for x, the weights on the host).
 *     workspace >= gnbv_linear_workspace_bytes(M, N, K). */
size_t gnbv_linear_workspace_bytes(int M, int N, int K);
int gnbv_linear_forward(const float *x, const float *w, const float *bias, int M, int N, int K, int relu, float *out,
                        void *workspace, size_t workspace_bytes, void *stream);

/*     Backward of the same layer (gennbv_amd/ops/encoder_ops.py::_LinearReluFn; the reference leaves it to autograd):
 *     g = d_out * (out > 0), dx = g w [M][K], dw = g^T x [N][K], db = sum_m g [N].  gnbv_linear_bwd_prep builds g's two operand
 *     images (row-scaled, split into f16 halves) in `workspace` and writes db (may be NULL); gnbv_linear_bwd_dx / _dw are the two
 *     products, each streaming its [.][K] operand once -- they may run on different streams once prep is done.
 *     M % 16 == 0, N % 16 == 0, N <= 256, K % 4 == 0, K >= 64; dx: M <= 128; dw: M <= 256.  fp32-accurate (split operands, fp32
 *     accumulation); |w| is clamped at 15.8 and |x| at 1015 like in the forward.  workspace 256-byte aligned. */
size_t gnbv_linear_bwd_workspace_bytes(int M, int N, int K);
int gnbv_linear_bwd_prep(const float *d_out, const float *out, int M, int N, float *db, void *workspace, size_t workspace_bytes,
                         void *stream);
int gnbv_linear_bwd_dx(const void *workspace, const float *w, int M, int N, int K, float *dx, void *stream);
int gnbv_linear_bwd_dw(const void *workspace, const float *x, int M, int N, int K, float *dw, void *stream);
/*     The same product, which also leaves sum(dw^2) as gnbv_linear_bwd_dw_sq_parts(K) fp64 partial sums (one per 64 columns) in
 *     `sq_partial`: the gradient-norm clip of the optimizer step (GnbvAdamStep.sq_partial) then needs no pass of its own over
 *     this -- by far the largest -- gradient. */
int gnbv_linear_bwd_dw_sq_parts(int K);
int gnbv_linear_bwd_dw_sq(const void *workspace, const float *x, int M, int N, int K, float *dw, double *sq_partial, void *stream);

/* B1  fc_grid with BatchNorm-2 + ReLU folded into its operand load (round 3; replaces Hybrid_Encoder.naive_encoder_grid[4:6] +
 *     output_layer_grid, gennbv/network/hybrid_encoder.py:40-49, as ONE product): x[m][k] = relu(scale[k / P] y[m][k] +
 *     shift[k / P]) is formed in registers from the conv stack's raw output y [M][K] (K = channels x P), the 4 K M bytes of
 *     normalised activations are never written or re-read.  Same arithmetic as gnbv_encoder_forward's k_bn_relu_apply followed by
 *     gnbv_linear_forward / gnbv_linear_bwd_dw_sq (one fma + one max in fp32, then the same split-f16 product): bit-identical
 *     results.  scale / shift: GnbvEncoderParams.bn_state + 4 x 16 and + 5 x 16 floats (layer 2) of the forward call that wrote
 *     y (features == NULL in gnbv_encoder_grid_forward skips that call's own BN2 + ReLU pass).  *range_flag (may be NULL): bit 4 when an
 *     operand passes 1000 (the f16 split clamps at 1015).  gnbv_linear_fold_ok: 1 when (M, N, K, P) can take this path
 *     (P >= 512, K % P == 0, split kernels on; both entry points refuse the others); otherwise materialise the activations
 *     (features != NULL) as before.
 *     d/dy of the product = the existing gnbv_linear_bwd_dx (d/dx) followed by gnbv_encoder_grid_backward (whose BN2 backward takes
 *     d/dx and y, never x). */
int gnbv_linear_fold_ok(int M, int N, int K, int P);
int gnbv_linear_forward_fold(const float *y, const float *scale, const float *shift, int P, int *range_flag, const float *w, const float *bias,
                             int M, int N, int K, int relu, float *out, void *workspace, size_t workspace_bytes, void *stream);
int gnbv_linear_bwd_dw_fold(const void *workspace, const float *y, const float *scale, const float *shift, int P, int M, int N, int K, float *dw,
                            double *sq_partial /*NULL: none*/, void *stream);


/* B1  pose-history input (gennbv/network/hybrid_encoder.py:63-74 positional_encoding with 2 frequency bands, :78-80): the state
 *     columns [0, 6 n_pose) of observation rows `rows` (NULL: rows 0 .. batch-1) of `base` (row stride in floats) ->
 *     out [batch][24 n_pose]: per pose cat(sin(p), cos(p)) of p = (x0, 2 x0, x1, 2 x1, ..., x5, 2 x5). */
int gnbv_pose_encode(const float *base, const int64_t *rows, int64_t row_stride, int batch, int n_pose, float *out, void *stream);

/* B1/B2  policy head, fused:  feat = relu([fa | fg] W_out^T + b_out)   Hybrid_Encoder.output_layer
 *                                                     (gennbv/network/hybrid_encoder.py:51-54, :89)
 *        logits = feat W_act^T + b_act, values = feat W_val^T + b_val      ActorCriticPolicy.action_net / value_net
 *                                                     (stable_baselines3/common/policies.py:975-979, :1011, :1024)
 *        fa [M][K1], fg [M][K2] (the two encoder branches, concatenated implicitly), W_out [F][K1+K2],
 *        W_act [A][F], W_val [1][F]; F, K1, K2 multiples of 16; torch.nn.Linear layouts.
 *        forward: feat [M][F] (kept for the backward), logits [M][A], values [M].
 *        backward: from d_logits [M][A], d_values [M]: d_fa, d_fg and the six parameter gradients
 *        (plain stores: pass the .grad slices for write-through).  dH_scratch: M*F floats. */
int gnbv_policy_head_forward(const float *fa, const float *fg, int M, int K1, int K2, const float *W_out, const float *b_out, int F,
                             const float *W_act, const float *b_act, int A, const float *W_val, const float *b_val, float *feat,
                             float *logits, float *values, void *stream);
int gnbv_policy_head_backward(const float *fa, const float *fg, int M, int K1, int K2, const float *feat, const float *d_logits,
                              const float *d_values, const float *W_out, int F, const float *W_act, int A, const float *W_val,
                              float *dH_scratch, float *d_fa, float *d_fg, float *gW_out, float *gb_out, float *gW_act,
                              float *gb_act, float *gW_val, float *gb_val, void *stream);

/* ------------------------------------------------------------------------- */
/* C2  TensorRolloutBuffer_Grid_Obs.compute_returns_and_advantage               */
/*     stable_baselines3/common/buffers.py:706-724.  All arrays [T,N] (the      */
/*     reference's [T,N,1]); episode_starts / dones are u8.                      */
/* ------------------------------------------------------------------------- */
int gnbv_gae_sb3(const float *rewards, const float *values, const uint8_t *episode_starts, const float *last_values,
                 const uint8_t *dones, int t_steps, int n, double gamma, double gae_lambda, float *advantages,
                 float *returns, void *stream);

/* C-alt  rsl_rl RolloutStorage.compute_returns (rsl_rl/storage/rollout_storage.py:130-142),
 *        advantages = returns - values, NOT yet normalised (:143-144 is the caller's reduction). */
int gnbv_gae_rsl(const float *rewards, const float *values, const uint8_t *dones, const float *last_values,
                 int t_steps, int n, double gamma, double lam, float *returns, float *advantages, void *stream);

/* ------------------------------------------------------------------------- */
/* C3/C4  minibatch gather + PPO loss + clip/Adam                               */
/*        stable_baselines3/common/buffers.py:753-762, ppo/ppo_grid_obs.py:196-275 */
/* ------------------------------------------------------------------------- */
/* rows [batch] int64 index the flattened [T*N] arrays (row = t*N + n). */
int gnbv_gather_minibatch(const int64_t *rows, int batch, int act_dim, const float *actions, const float *values,
                          const float *log_probs, const float *advantages, const float *returns, float *o_actions,
                          float *o_values, float *o_log_probs, float *o_adv, float *o_ret, void *stream);

/* One launch (one wave per sample; the workgroup that finishes last adds the per-sample terms in a fixed order):
 * advantage normalisation, MultiCategorical log-prob / entropy, clipped surrogate,
 * clipped value loss, entropy loss, loss = policy_scale*pg + ent_coef*ent + vf_coef*vl,
 * approx-KL, clip fraction, and d loss / d logits, d loss / d values.
 * stats row (8 floats) = pg, vl, ent, approx_kl, clip_fraction, loss, live, 0 is written at
 * stats[*stats_row] and *stats_row is incremented; *stop_flag becomes 1 (sticky) when
 * approx_kl > 1.5*target_kl (target_kl <= 0: never). [host struct, device pointers] */
typedef struct GnbvPpoLoss {
    int batch, n_logits, n_heads;
    int head_dims[8];
    int normalize_advantage;
    float clip_range, clip_range_vf /* <= 0: no value clipping */, ent_coef, vf_coef, policy_scale, target_kl;
    const float *logits;        /* [B, n_logits] */
    const float *values;        /* [B] */
    const float *actions;       /* [B, n_heads] stored as float like the reference buffer */
    const float *old_values, *old_log_prob, *advantages, *returns; /* [B] */
    float *d_logits;            /* out [B, n_logits] */
    float *d_values;            /* out [B] */
    float *head_entropy;        /* out [B, n_heads] or NULL */
    float *head_lse;            /* out [B, n_heads] or NULL */
    float *stats;               /* [rows, 8] */
    int64_t *stats_row;         /* in/out [1] */
    int *stop_flag;             /* in/out [1] or NULL */
    float *scratch;             /* [8*B + 64] device scratch, ZERO-initialised by the caller once (holds a completion
                                   counter that every call leaves at zero) */
    float *kl_out;              /* NULL, or [1]: receives approx_kl INSTEAD of setting stop_flag
                                   (data-parallel: decided on the global mean, gnbv_clip_adam_step) */
    const int64_t *rows;        /* NULL, or [B]: fused minibatch gather (buffers.py:753-762) -- actions, old_values,
                                   old_log_prob, advantages, returns then point at the whole [T*N] rollout arrays
                                   and sample i reads row rows[i] */
    const float *adv_norm;      /* NULL: the minibatch's own advantage mean / unbiased std (ppo_grid_obs.py:214-216);
                                   or [2] = (mean, 1 / (std + 1e-8)) of the GLOBAL minibatch (data-parallel replicas:
                                   the statistics of all ranks' rows, gennbv_amd/parallel.py) */
    int defer_stats;            /* 0: gnbv_ppo_loss also writes the statistics row and takes the KL stop decision (its last workgroup:
                                   a release fence + a ticket per workgroup on the update's critical path).  1: it only leaves the
                                   per-sample terms in `scratch`; the caller finishes them with gnbv_ppo_loss_finish, or -- no launch
                                   of its own -- inside gnbv_clip_adam_step_ex (GnbvAdamStep.loss_finish), before the update reads
                                   the stop flag.  With kl_out (data-parallel replicas: the rank's KL must exist before the all-reduce
                                   that carries it) only gnbv_ppo_loss_finish, launched in front of that exchange -- e.g. on a second
                                   stream beside the backward (sb3/ppo_grid_obs.py _dp_step_body). */
} GnbvPpoLoss;

int gnbv_ppo_loss(const GnbvPpoLoss *args /*[host]*/, void *stream);
int gnbv_ppo_loss_finish(const GnbvPpoLoss *args /*[host]; defer_stats == 1*/, void *stream);

/* Soft-target imitation loss (gennbv_amd/sb3/imitation.py): k weighted candidate action tuples per sample -- a planner's scores over
 * its k candidates -- against the policy's MultiCategorical heads.  ONE launch, one wave per sample.  For sample b with source row
 * r = rows ? rows[b] : b, w_b = sample_w ? sample_w[r] : 1, candidate weights q_j = cand_w ? cand_w[r,j] : [j == 0], Q = sum_j q_j:
 *   dead, flags |= 2 : w_b or any q_j negative or non-finite;
 *   else dead        : w_b == 0 or Q == 0;
 *   else dead, flags |= 1 : a candidate with q_j != 0 has an index outside [0, head_dims[h]) (a candidate of weight 0 is not judged).
 * A dead sample gets a zero d_logits row and a zero d_values element and enters no sum.  For a live sample, per head h of n categories:
 *   m_h[c] = (1 - label_smoothing) * sum_j (q_j / Q) [cand[r,j,h] == c] + label_smoothing / n   (added in candidate order)
 *   lp_h = log_softmax, p_h = exp(lp_h), H_h = -sum p lp, ce_b = -sum_h sum_c m_h[c] lp_h[c]
 *   W = sum of w_b over the live samples
 *   loss = (1/W) sum_b w_b (ce_b - ent_coef sum_h H_h + vf_coef (v_b - R_r)^2)
 *   d_logits[b,h,c] = (w_b/W) ((p - m) + ent_coef p (lp + H_h)),  d_values[b] = (w_b/W) 2 vf_coef (v_b - R_r)
 * A head of one category contributes nothing (zero gradient).  values == NULL: no value term; returns == NULL: (v - R) counts as 0.
 * stats row (8 floats, at stats[*stats_row], then *stats_row += 1) = weighted mean ce, weighted mean (v - R)^2, weighted mean
 * sum_h H_h, agreement (share of live samples whose first arg-max equals candidate j* on every head of more than one category;
 * j* = the first candidate of the largest weight), mean over live samples of -sum_h lp_h[cand[r,j*,h]], loss, live count, 0.
 * W == 0: every output is zero and the row is zero.  Every element of d_logits (and d_values) is written on every call; all sums,
 * W included, are added in one fixed order by the workgroup that finishes last, which also applies 1/W: deterministic, independent
 * of the grid, and with `rows` bit-identical to the call on gathered arrays.  No workspace beyond `scratch`, no allocation, no host
 * synchronisation.  Returns hipErrorInvalidValue, before any launch, for a value outside the ranges below, a NULL logits, cand,
 * d_logits, stats, stats_row, flags or scratch, values without d_values, or values with vf_coef > 0 without returns.
 * [host struct, device pointers] */
typedef struct GnbvImitationLoss {
    int batch, n_logits, n_heads; /* batch >= 1, n_heads 1..8 */
    int head_dims[8];             /* each 1..1024, sum == n_logits */
    int k;                        /* candidates per sample, >= 1 */
    float label_smoothing /* [0,1) */, ent_coef /* >= 0 */, vf_coef /* >= 0 */;
    const float *logits;          /* [B, n_logits] */
    const float *values;          /* [B] or NULL */
    const int64_t *cand;          /* [R, k, n_heads] */
    const float *cand_w;          /* [R, k] or NULL: candidate 0 alone carries weight 1 */
    const float *sample_w;        /* [R] or NULL: 1 */
    const float *returns;         /* [R] or NULL */
    const int64_t *rows;          /* [B] or NULL: fused gather, sample b reads source row rows[b]; NULL: row b */
    float *d_logits;              /* out [B, n_logits] */
    float *d_values;              /* out [B]; required iff values != NULL */
    float *stats;                 /* [rows, 8] */
    int64_t *stats_row;           /* in/out [1] */
    int *flags;                   /* in/out [1], sticky: bit 0 index out of range, bit 1 bad weight */
    float *scratch;               /* [8*B + 64], ZERO-initialised by the caller once (per-sample terms + a completion counter
                                     that every call leaves at zero) */
} GnbvImitationLoss;
int gnbv_imitation_loss(const GnbvImitationLoss *args /*[host]*/, void *stream);

/* C5  rollout side of MultiCategoricalDistribution (stable_baselines3/common/distributions.py:299-352 via
 *     ActorCriticPolicy.forward, policies.py:1024-1030): actions[b][h] ~ Categorical(softmax(logits_h[b])) by
 *     the inverse CDF at uniforms[b][h] in [0,1) (deterministic != 0: first arg-max = mode()), and
 *     log_prob[b] = sum_h log softmax(logits_h[b])[actions[b][h]].  head_dims [n_heads] is a HOST array,
 *     sum(head_dims) == n_logits, n_heads <= 8.  Same distribution as torch.multinomial, different random stream. */
int gnbv_multicategorical_sample(const float *logits, int batch, int n_logits, int n_heads, const int *head_dims /*[host]*/,
                                 const float *uniforms, int deterministic, int64_t *actions, float *log_prob, void *stream);

/* rsl_rl flavour of the PPO minibatch loss (rsl_rl/algorithms/ppo.py:160-180): scalar part of
 *   surrogate  = mean(max(-A r, -A clamp(r, 1 - c, 1 + c))),  r = exp(log_prob - old_log_prob)
 *   value_loss = mean(max((v - R)^2, (tv + clamp(v - tv, -c, c) - R)^2))   (use_clipped_value_loss) or mean((R - v)^2)
 *   loss       = surrogate + value_loss_coef * value_loss - entropy_coef * mean(entropy)
 * for ANY action distribution: the caller evaluates log_prob / value / entropy of the minibatch with its own modules and
 * back-propagates the three gradient vectors this call returns (ties of max() split evenly, like torch.max).
 * All arrays [batch] fp32, device.  sums [2] (device, caller-zeroed): += value_loss, += surrogate (the reference's
 * running `mean_value_loss` / `mean_surrogate_loss`, read once per update() instead of two .item() per minibatch). */
int gnbv_ppo_loss_rsl(int batch, const float *log_prob, const float *old_log_prob, const float *advantages, const float *values,
                      const float *target_values, const float *returns, float clip_param, float value_loss_coef,
                      float entropy_coef, int use_clipped_value_loss, float *d_log_prob, float *d_values, float *d_entropy,
                      float *sums, void *stream);

/* torch.nn.utils.clip_grad_norm_(max_grad_norm) + torch.optim.Adam step over ONE flat fp32
 * buffer of n parameters (max_grad_norm <= 0: no clipping). grads is the SUM over ranks,
 * grad_scale = 1/world turns it into the mean (1.0 on one GPU).  kl_slot (may be NULL): sum over
 * ranks of approx_kl; *stop_flag becomes 1 (sticky) when kl_slot*grad_scale > 1.5*target_kl.
 * *step is incremented and the update applied unless *stop_flag != 0.
 * norm_out[0] = norm of the mean gradient, [1] = factor applied to `grads`. */
size_t gnbv_adam_workspace_bytes(void);
int gnbv_clip_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float max_grad_norm,
                        float lr, float beta1, float beta2, float eps, int64_t *step, int *stop_flag, float grad_scale,
                        const float *kl_slot, float target_kl, float *norm_out, void *workspace, size_t workspace_bytes,
                        void *stream);
/* Same, for a minibatch update that is replayed as a hipGraph (the reference's inner loop, ppo_grid_obs.py:199-287, walks
 * `rollout_buffer.get(batch_size)`): the Adam launch -- the last of a minibatch -- also copies row (*counter + 1) % table_rows of
 * `table` [table_rows][row_len] (the row numbers of every minibatch of this train() call) into `out`, the buffer all kernels
 * of the graph read their row numbers from, and stores the new *counter: no copy and no host work between two replays. */
int gnbv_clip_adam_step_rotate(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float max_grad_norm,
                               float lr, float beta1, float beta2, float eps, int64_t *step, int *stop_flag, float grad_scale,
                               const float *kl_slot, float target_kl, float *norm_out, void *workspace, size_t workspace_bytes,
                               const int64_t *table, int table_rows, int row_len, int64_t *out, int *counter, void *stream);
/* Both of the above are this call with the optional parts left out.  `table` .. `counter`: the row rotation of
 * gnbv_clip_adam_step_rotate (table == NULL: none).  sq_lo .. sq_parts: the squared sum of the gradient slice [sq_lo, sq_hi) was
 * already taken by its producer (gnbv_linear_bwd_dw_sq) and is read from `sq_partial` instead of from the gradient itself;
 * sq_partial == NULL: the whole gradient is summed here.  Two launches: the squared-norm partial sums (+ step counter / KL
 * decision), then the update, every workgroup of which evaluates the clip coefficient from the partial sums in one fixed order. */
typedef struct GnbvAdamStep {
    float *params; const float *grads; float *exp_avg, *exp_avg_sq; int64_t n;
    float max_grad_norm, lr, beta1, beta2, eps;
    int64_t *step; int *stop_flag; float grad_scale; const float *kl_slot; float target_kl;
    float *norm_out; void *workspace; size_t workspace_bytes;
    const int64_t *table; int table_rows, row_len; int64_t *out; int *counter;
    int64_t sq_lo, sq_hi; const double *sq_partial; int sq_parts;
    const GnbvPpoLoss *loss_finish;     /* NULL, or [host] the loss arguments of this minibatch with defer_stats = 1: an extra workgroup
                                           of the norm launch adds up its per-sample terms (statistics row, KL stop decision, then the
                                           step counter) -- same stop_flag as this call's */
    int64_t upd_skip_lo, upd_skip_hi;   /* parameters [upd_skip_lo, upd_skip_hi) are NOT updated by this call (their gradient still
                                           counts for the norm through sq_partial): a slice whose update is sharded over the
                                           data-parallel replicas, gnbv_adam_shard_step */
} GnbvAdamStep;
int gnbv_clip_adam_step_ex(const GnbvAdamStep *a /*[host]*/, void *stream);
/* sum(grads[0 .. n)^2) as gnbv_sq_partials_count() fp64 partial sums in one fixed order -> partial [device].  The sharded data-parallel
 * update: a rank squares the shard of the reduced gradient it owns, the partial sums are summed over the ranks (an all-reduce of
 * 2 KB) and enter the clip factor of gnbv_clip_adam_step_ex through GnbvAdamStep.sq_partial / sq_parts. */
int gnbv_sq_partials_count(void);
int gnbv_sq_partials(const float *grads, int64_t n, double *partial /*[gnbv_sq_partials_count()]*/, void *stream);
/* Adam on a shard of n parameters with the clip factor norm_out[1] that gnbv_clip_adam_step_ex of the SAME optimizer step left
 * behind (same step counter and stop flag, neither is modified). */
int gnbv_adam_shard_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, const float *norm_out,
                         float lr, float beta1, float beta2, float eps, const int64_t *step, const int *stop_flag, void *stream);


/* ------------------------------------------------------------------------- */
/* 8f.3  evaluation metric: reconstruction accuracy of Env_Eval_GenNBV          */
/*       (gennbv/env/env_eval_gennbv.py:253-262): pytorch3d.loss.chamfer_distance */
/*       (x[None], y[None])[0] with pytorch3d 0.7.8 defaults = mean_i min_j |x_i-y_j|^2 */
/*       + mean_j min_i |x_i-y_j|^2 (squared distances).  x [n,3], y [m,3] fp32.  */
/* ------------------------------------------------------------------------- */
size_t gnbv_chamfer_workspace_bytes(int n, int m);
int gnbv_chamfer_distance(const float *x, int n, const float *y, int m, float *out /*[1]*/, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* 8f.3 on the device (new entry points of ABI 5): the per-episode scan set of  */
/*      Env_Eval_GenNBV (env_eval_gennbv.py:156-164, reset_idx :321-322) and     */
/*      its accuracy (:253-263), batched over envs, no host synchronisation.     */
/* ------------------------------------------------------------------------- */
/* The set of env e is its 1 cm keys: per axis k = rint(fp32(p * 100.0f)) (half to even, torch.round) of every foreground
 * point of the A1/A2 chain (gnbv_post_process_depth + gnbv_back_projection, same fp32 order), |k| < 2^20.  Storage is
 * caller-owned, gnbv_scan_set_bytes(n, capacity) bytes in all: table [n, capacity] u64 filled with all-ones bytes (empty),
 * keys [n, capacity] u64 (the unique keys, append order), counts [n] i32 = 0, flags [n] i32 = 0.  capacity = the most unique
 * keys an env can hold, a multiple of 64 below 2^31.  flags[e] bit 0: a key found no free slot (overflow), bit 1: a
 * foreground point was non-finite or |k| >= 2^20; such points are not added and the flags stay set until the caller
 * clears them.  [host struct] */
typedef struct GnbvScanSet {
    int n;
    int64_t capacity;
    uint64_t *table;
    uint64_t *keys;
    int32_t *counts;
    int32_t *flags;
} GnbvScanSet;

/* The GT clouds, static: env e's m_e > 0 points, ordered spatially (any order: gennbv_amd/eval/scan_accumulator.py sorts
 * them by Morton code), pts [M] float4 (x, y, z, unused) at pt_start[e] .. pt_start[e+1] - 1, orig[i] = index of point i in
 * the env's given order; a tree per env in heap layout: P = pow2[e] (a power of two >= ceil(m_e / 32)), nodes
 * node_start[e] .. node_start[e] + 2P - 1, each two float4 (lo, hi): node P + j = the box of points 32 j .. 32 j + 31,
 * node i < P = the union of nodes 2i and 2i+1, a node without points = (+inf, -inf).  Every pointer device. [host struct] */
typedef struct GnbvScanGt {
    int n;
    int64_t num_points;             /* M = pt_start[n] */
    const int64_t *pt_start;        /* [n+1] */
    const float *pts;               /* [M, 4] */
    const int32_t *orig;            /* [M] */
    const int64_t *node_start;      /* [n] */
    const int32_t *pow2;            /* [n] */
    const float *nodes;             /* [sum 2P, 2, 4] */
} GnbvScanGt;

size_t gnbv_scan_set_bytes(int n, int64_t capacity);
/* One env step: add every env's foreground keys of depth_raw / seg_raw [n, h, w] (raw, as rendered) under c2w [n, 4, 4].
 * One launch; no workspace. */
int gnbv_scan_add_frame(const GnbvScanSet *set /*[host]*/, const float *depth_raw, const float *seg_raw, const float *c2w,
                        const float *inv_intri /*[host] [3,3]*/, int h, int w, float depth_sense_dist, void *stream);
/* Empty the sets of the envs with mask[e] != 0 (u8 [n], e.g. reset_buf).  One launch; no workspace; flags are kept. */
int gnbv_scan_clear(const GnbvScanSet *set /*[host]*/, const uint8_t *mask, void *stream);
/* Workspace of gnbv_scan_score and gnbv_scan_export (256-B aligned), M = the GT points of all envs (0 for export only). */
size_t gnbv_scan_workspace_bytes(int n, int64_t capacity, int64_t gt_points);
/* For every env with mask[e] != 0, scored[e] == 0, counts[e] > 0 and flags[e] == 0: accuracy[e] = fp32(fp32(cd) * 100.0f),
 * cd = mean_i min_j |x_i - y_j|^2 + mean_j min_i |x_i - y_j|^2 (gnbv_chamfer_distance's formula and sums) over the set's
 * points x = fp32(k) * 0.01f and the env's GT cloud y, and scored[e] = 1.  The minima are exact (the brute force's fp32
 * values); the sums are fp64 in a fixed order (GT side: given order, bit-identical to gnbv_chamfer_distance; scanned side:
 * Morton order of the keys), so the result is deterministic and within 2 fp32 ulps of gnbv_chamfer_distance x 100 over the
 * lexicographically sorted points.  Other envs are untouched.  Sorts the key list of the scored envs in place. */
int gnbv_scan_score(const GnbvScanSet *set /*[host]*/, const GnbvScanGt *gt /*[host]*/, const uint8_t *mask, float *accuracy /*[n]*/,
                    int32_t *scored /*[n]*/, void *workspace, size_t workspace_bytes, void *stream);
/* Env `env`'s set as rows fp32(k) * 0.01f in lexicographic order (== torch.unique(torch.round(pts, decimals=2), dim=0) of the
 * points added since its last clear): xyz [counts[env], 3].  The set is not modified. */
int gnbv_scan_export(const GnbvScanSet *set /*[host]*/, int env, float *xyz, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* View gain (a new entry point of ABI 5): how much would env e's map change    */
/* if its camera went to candidate pose j?  The voxel update's ray model run     */
/* hypothetically against the tri-class grid, K candidates per env.              */
/* ------------------------------------------------------------------------- */
/* Env e holds tri [g,g,g] int8 (C order x, y, z; < 0 free, 0 unknown, > 0 occupied).  Candidate pose (x, y, z, roll, pitch,
 * yaw), env-local:
 *   - c2w = gnbv_render_depth's camera matrix of the pose (fp64 trig rounded to fp32, roll ignored);
 *   - rays: the pixels u = stride/2 + i stride < w, v = stride/2 + j stride < h (integer division);
 *   - the ray of (u, v) ends at the world point gnbv_back_projection gives that pixel at depth `range` (the canonical fp32
 *     chain); source voxel = gnbv_pose_to_idx(x, y, z), target voxel = gnbv_pose_to_idx(end point), both unclamped (voxel
 *     coordinates beyond +-2^24 saturate there);
 *   - the ray visits the in-grid voxels of gnbv_bresenham3d's line from source to target in order and stops in front of the
 *     first occupied one (not counted); a ray that met one is `blocked`.
 * gain[e, j] = { distinct unknown voxels visited by any ray, the same over the blocked rays only, blocked rays }.  Integers
 * with one right answer; every element is written; deterministic (no global atomics).  One launch, no workspace.
 * g outside 2..64 (the grid and two visited masks live in LDS; gnbv_view_gain_slab below goes to 128), stride < 1, range not
 * positive and finite, or k < 1 return hipErrorInvalidValue.  [host struct]; pointers are device unless noted. */
typedef struct GnbvViewGain {
    int n, k, g;                    /* envs, candidates per env, grid edge */
    const int8_t *tri_i8;           /* [n, g^3] with a row stride in BYTES (rows inside a larger buffer work) */
    int64_t tri_row_stride;
    const float *poses;             /* [n, k, 6] contiguous */
    const float *range_gt;          /* [n, 6] */
    const float *voxel_size;        /* [n, 3] */
    const float *inv_intri;         /* [host] [3,3] the updater's inverse intrinsics */
    int h, w, stride;               /* camera and the pixel lattice's step */
    float range;                    /* metres */
    int32_t *gain;                  /* [n, k, 3] */
    float *c2w_out;                 /* [n, k, 4, 4] the matrices used, or NULL */
    int chunk;                      /* candidates per workgroup, 0 = chosen from n and k (any value gives the same result) */
    int ablate;                     /* measurements only, 0 otherwise: bit 0 walk without marking (the counts are then 0),
                                     * bit 1 no second mask (unknown_hit is then 0) */
    /* the view gain of a MEASURED frame (below); all zero / NULL: the rule above, bit for bit */
    const float *depth_raw;         /* raw camera depth as gnbv_render_depth writes it, or NULL: candidate j of env e reads
                                     * [h, w] floats, row-major, at depth_raw + e depth_env_stride + j depth_cand_stride */
    int64_t depth_env_stride, depth_cand_stride; /* in floats, >= h w; a candidate stride of 0 is legal with k == 1 */
    float depth_sense_dist;         /* the updater's value: negative and finite */
    int8_t *carve_i8;               /* [n, g^3] with a row stride in BYTES (>= g^3), or NULL; only with depth_raw */
    int64_t carve_row_stride;
} GnbvViewGain;
int gnbv_view_gain(const GnbvViewGain *args /*[host]*/, void *stream);

/* The view gain of a measured frame: what the frame revealed.  With args->depth_raw != NULL every one of the four entry points
 * gnbv_view_gain, gnbv_view_gain_masks, gnbv_view_gain_slab and gnbv_view_gain_slab_masks ends the ray of lattice pixel (u, v) by
 * the pixel's raw depth r instead of by `range`:
 *   - the ray is SURFACE-ENDED iff r is finite, r != 0, r > depth_sense_dist and |r| <= range; its length is then |r|, exactly the
 *     depth gnbv_voxel_update's A1 gives that pixel;
 *   - every other ray is RANGE-ENDED with length `range`: -inf, NaN, +-0, a value at or below the clamp, a hit beyond `range`;
 *   - the ray ends at the world point gnbv_back_projection gives the pixel at that length; source voxel, target voxel, the line,
 *     its in-grid voxels in order and the stop in front of the first occupied voxel are gnbv_view_gain's, unchanged;
 *   - on a surface-ended ray a visited voxel equal to the ray's target voxel is not marked and not counted: a surface is there.
 *     On a range-ended ray it is a voxel like any other.
 * gain, unknown_bits, hit_bits and c2w_out keep their meaning and layouts over this ray set.  carve_i8[e, lin] = -1 for every
 * voxel of U(e, j) of any candidate j: plain byte stores of one value, and no other byte of the row is touched.  carve_i8 may be
 * tri_i8 (same pointer, same stride) with k == 1 in gnbv_view_gain / _masks, where one workgroup owns the env and packs the row
 * before it stores, and with any k in the slab entry points, where the first kernel packs every row.  The kernels are compile-time
 * variants of their own: a call without depth_raw runs the code it ran before.  Deterministic, no global atomics beyond those of
 * gnbv_view_gain_slab / _masks, no workspace growth, no allocation, no host synchronisation; `chunk` and `slab` do not change
 * the result.
 * Returns hipErrorInvalidValue, before any launch, also for: a depth stride below h w (a candidate stride of 0 with k > 1
 * included), depth_sense_dist not finite or >= 0, carve_i8 without depth_raw, with ablate != 0 or with a row stride below g^3,
 * and any other overlap of carve_i8 and tri_i8.  The test is made on the two SPANS [base, base + (n - 1) stride + g^3), not row
 * by row: interleaved rows that are pairwise disjoint (carve_i8 = tri_i8 + g^3 with both strides 2 g^3) are refused too. */

/* gnbv_view_gain that keeps the sets it counts (a new entry point of ABI 5).  Rays, camera, source and target voxels, walk and
 * stop rule are gnbv_view_gain's, unchanged.  For env e and candidate j, U(e, j) = the distinct unknown voxels visited by any ray
 * before its first occupied voxel, H(e, j) (a subset of U) the same over the blocked rays only; a voxel is lin = (x g + y) g + z.
 *   unknown_bits[e, j, :]: bit lin & 31 of word lin >> 5 is set iff lin is in U(e, j);  hit_bits[e, j, :] holds H(e, j) the same
 * way: rows of `words` words, unswizzled -- gnbv_cover_greedy's mask_bits layout and the updater's scanned_bits'
 * (words = gnbv_grid_bit_words(g) is always legal).  Every word of every row of a non-NULL output is written on every call, the
 * zero words and the pad words from ceil(g^3 / 32) up to `words` included: the caller zeroes nothing.  args->gain is required and
 * filled exactly as gnbv_view_gain fills it, so popcount(unknown_bits[e, j]) == gain[e, j, 0] and popcount(hit_bits[e, j]) ==
 * gain[e, j, 1]; c2w_out as there.  One launch: the workgroup of (env, chunk) owns its candidates' rows and stores them from its
 * LDS masks with 16-byte stores before it clears them.  No global atomics, no workspace, no allocation, no host synchronisation;
 * deterministic; the result depends neither on `chunk` nor on which outputs are requested.
 * Returns hipErrorInvalidValue for everything gnbv_view_gain refuses (g outside 2..64 included), both outputs NULL, `words` not
 * a multiple of 4 or < ceil(g^3 / 32), an output that is not 16-byte aligned, n k words > 2^31 - 1, and args->ablate != 0. */
int gnbv_view_gain_masks(const GnbvViewGain *args /*[host]*/, int words, int32_t *unknown_bits /*[n, k, words] or NULL*/,
                         int32_t *hit_bits /*[n, k, words] or NULL*/, void *stream);

/* The same quantity, bit for bit, for 2 <= g <= 128 (new entry points of ABI 5).  The grid no longer fits in LDS, so the call
 * runs three kernels per batch of envs on the caller's stream: the grids packed to 2 bits per voxel and the cameras; every
 * ray's fate (where it enters the grid, where it stops; `blocked` is complete here); then workgroups (env, chunk of candidates,
 * slab of `slab` x-planes) mark the slab's part of the two visited masks in LDS and add their distinct counts to gain with
 * int32 atomicAdd: integer sums, so the result is deterministic and does not depend on `slab` (0 = chosen from g: 16 at 128^3;
 * a height whose grid + masks exceed a workgroup's LDS is reduced to the largest that fits, 19 at 128^3) or on `chunk`.
 * Every element of gain is written.  No host synchronisation, no allocation.
 * The workspace (16-B aligned, caller-owned, reused by every call) holds ONE batch of envs: 20 bytes per ray (n_b k rays),
 * g^3 / 4 bytes per env and 80 bytes per candidate, n_b = the envs whose ray records fill 128 MiB (at least 8, at most n), so
 * it stops growing with n: 155 MB at 512 envs x 128^3, 240x320, stride 4, k = 32 (n_b = 43), where one batch for all envs
 * would take 1.57 GB of records and 268 MB of grids.
 * Returns hipErrorInvalidValue for everything gnbv_view_gain refuses (with g up to 128), slab < 0, and a NULL, misaligned or
 * too small workspace; gnbv_view_gain_slab_workspace_bytes returns 0 for sizes the call would refuse. */
size_t gnbv_view_gain_slab_workspace_bytes(int n, int k, int g, int h, int w, int stride);
int gnbv_view_gain_slab(const GnbvViewGain *args /*[host]*/, int slab, void *workspace, size_t workspace_bytes, void *stream);

/* gnbv_view_gain_slab that keeps the sets it counts: gnbv_view_gain_masks for 2 <= g <= 128 (a new entry point of ABI 5).
 * U(e, j), H(e, j), the row layout (bit lin & 31 of word lin >> 5, lin = (x g + y) g + z, rows of `words` words, unswizzled)
 * and the rule that every word of every row of a non-NULL output is written on every call -- the zero words, the pad words from
 * ceil(g^3 / 32) up to `words`, the rows no ray reaches and the call without any ray (stride / 2 >= w or h) included -- are
 * gnbv_view_gain_masks'; a row belongs to env e of all n, whatever batch of the workspace computed it.  args->gain is required
 * and filled exactly as gnbv_view_gain_slab fills it, so popcount(unknown_bits[e, j]) == gain[e, j, 0] and
 * popcount(hit_bits[e, j]) == gain[e, j, 1]; c2w_out as there.  The same three kernels per batch of envs: a slab workgroup
 * stores its part of both LDS masks into the candidate's rows before it clears them (16-byte stores; 4-byte stores at the slab's
 * ragged ends); a row word that two slabs share, where slab g^2 is not a multiple of 32, is zeroed by the first kernel and
 * gets both parts by atomicOr -- disjoint bit sets, so the result is deterministic and depends neither on `slab` (chosen and
 * reduced as in gnbv_view_gain_slab; the LDS masks may take 16 bytes more each), nor on `chunk`, nor on which outputs are
 * requested.  The workspace is gnbv_view_gain_slab_workspace_bytes, unchanged.  No host synchronisation, no allocation.
 * Returns hipErrorInvalidValue, before any launch, for everything gnbv_view_gain_slab refuses (g outside 2..128 included),
 * args->ablate != 0, both outputs NULL, `words` not a positive multiple of 4 or < ceil(g^3 / 32), an output that is not 16-byte
 * aligned, and n k words > 2^31 - 1. */
int gnbv_view_gain_slab_masks(const GnbvViewGain *args /*[host]*/, int slab, void *workspace, size_t workspace_bytes, int words,
                              int32_t *unknown_bits /*[n, k, words] or NULL*/, int32_t *hit_bits /*[n, k, words] or NULL*/,
                              void *stream);

/* ------------------------------------------------------------------------- */
/* View coverage (a new entry point of ABI 5): which ground-truth voxels would  */
/* the voxel update mark if env e's camera stood at candidate pose j?  The      */
/* renderer's trace and the update's back-projection, fused: no image is stored. */
/* ------------------------------------------------------------------------- */
/* For env e of `scene`, candidate pose (x, y, z, roll, pitch, yaw), env-local, and the pixel-lattice step `stride`:
 *   - c2w = gnbv_render_depth's camera matrix of the pose, bit for bit (fp64 trig rounded to fp32, roll ignored);
 *   - pixels u = stride/2 + i stride < w, v = stride/2 + j stride < h (integer division, as gnbv_view_gain); stride 1 is every pixel;
 *   - the pixel's (depth_raw, seg_raw) is exactly what gnbv_render_depth writes for that env, camera and pixel (one shared
 *     trace: csrc/raytrace.h); the pixel is foreground iff it hits an object (seg 255, the update's seg > 50);
 *   - a foreground pixel's world point is the update's: the depth clamp of gnbv_post_process_depth with depth_sense_dist, the
 *     canonical fp32 chain of gnbv_back_projection; it is kept under gnbv_points_to_idx's strict bounds and mapped to its
 *     voxel floor(RN((p - vmin) / v)) clamped to [0, g-1];
 *   - S(e, j) = the distinct voxels of the kept foreground points.  At stride 1 with the env's own h, w, inverse intrinsics
 *     and sense distance, S is exactly the hit mask gnbv_update_occ_grid* forms from that view, and S & gt & ~scanned is
 *     exactly what it adds to scanned_bits.
 * cover[e, j] = { |S & gt & ~scanned|, |S & gt|, kept foreground lattice pixels }: integers with one right answer, every
 * element written on every call.  seen_bits[e] |= S & gt over all k candidates (device-scope atomicOr of the non-zero words;
 * the caller zeroes it, or keeps accumulating).  The bit layout is gnbv_pack_grid_bits' (bit v = voxel (x*g+y)*g+z, rows of
 * gnbv_grid_bit_words(g) words, 16-byte aligned).  One workgroup per (env, chunk of candidates) keeps S in LDS (g <= 105:
 * up to 144 KiB); above, the words are split into windows of `window` words and the per-window counts are added with int32
 * atomicAdd after a zeroing launch -- integer sums, so the result depends neither on `chunk` nor on `window`.  Deterministic.  No host
 * synchronisation, no allocation, no workspace.
 * Returns hipErrorInvalidValue for g outside 2..128, n outside 1..65535, stride < 1, k < 1, h or w outside 1..32768, chunk or window < 0, cover
 * and seen_bits both NULL, a NULL required pointer (scene, poses, range_gt, voxel_size, inv_intri, gt_bits, the scene's cell
 * arrays), a misaligned bit row, or scene->n != n.  [host struct]; pointers are device unless noted. */
typedef struct GnbvViewCover {
    int n, k, g;                    /* envs (== scene->n), candidates per env, grid edge */
    const float *poses;             /* [n, k, 6] contiguous */
    const float *range_gt;          /* [n, 6] */
    const float *voxel_size;        /* [n, 3] */
    const float *inv_intri;         /* [host] [3,3] the updater's inverse intrinsics */
    int h, w, stride;               /* camera and the pixel lattice's step */
    float depth_sense_dist;         /* the updater's (negative: depth_raw is clamped from below), e.g. -50 */
    const int32_t *gt_bits;         /* [n, words], words = gnbv_grid_bit_words(g) */
    const int32_t *scanned_bits;    /* [n, words], or NULL = nothing scanned */
    int32_t *cover;                 /* [n, k, 3] (new_gt, seen_gt, hits), or NULL */
    int32_t *seen_bits;             /* [n, words], or NULL */
    int chunk;                      /* candidates per workgroup, 0 = chosen from n and k (any value gives the same result) */
    int window;                     /* bit-set words per workgroup, 0 = chosen from g (the fewest windows that fit the LDS; any
                                     * value gives the same result; rounded up to 4, reduced to what fits) */
} GnbvViewCover;
int gnbv_view_cover(const GnbvMeshScene *scene /*[host]*/, const GnbvViewCover *args /*[host]*/, void *stream);

/* ------------------------------------------------------------------------- */
/* View pool (new entry points of ABI 5): every candidate's visible ground     */
/* truth as a bit mask, traced once, and greedy set cover on those masks.      */
/* ------------------------------------------------------------------------- */
/* mask_bits[e, j, :] = S(e, j) & gt_bits[e, :], S exactly gnbv_view_cover's seen set of the same arguments; rows of
 * words = gnbv_grid_bit_words(g).  Every word of every row is written on every call, the zero words and the pad words past the
 * voxels included: the caller does not zero mask_bits.  The workgroup of (env, chunk[, window]) owns its window's words of its
 * candidates' rows and stores them from the LDS bit set with 16-byte stores before it clears the set (the workgroup of the last
 * window also stores the pad words): no atomics and no zeroing launch for the masks, so the result depends neither on `chunk` nor
 * on `window`.  args->cover and args->seen_bits may both be NULL here; a non-NULL one is filled exactly as gnbv_view_cover fills
 * it (popcount(mask & ~scanned) == cover[.., 0], popcount(mask) == cover[.., 1]).  Deterministic.  No host synchronisation, no
 * allocation, no workspace.
 * Returns hipErrorInvalidValue for a NULL or not 16-byte aligned mask_bits and for everything gnbv_view_cover refuses, except
 * that cover and seen_bits may both be NULL. */
int gnbv_view_cover_masks(const GnbvMeshScene *scene /*[host]*/, const GnbvViewCover *args /*[host]*/,
                          int32_t *mask_bits /*[n, k, words]*/, void *stream);

/* Greedy set cover over per-candidate bit masks (gnbv_view_cover_masks' layout, or any [n, k, words] rows).  Per env, with
 * covered = covered_in (NULL: empty), for round t = 0 .. rounds-1:
 *   g_j = popcount(mask[j] & ~covered);  score_j = contact[j] ? -1 : g_j;
 *   j* = the largest score, ties to the lowest j (all candidates in contact: j* = 0);
 *   choice[t] = j*;  gain[t] = g_j* (the true gain, also of a contact winner);  covered |= mask[j*].
 * A candidate may win again with gain 0.  Integers with one right answer.  gains0[e, j] = g_j of round 0 for every candidate.
 * lazy = 1 evaluates only the candidates whose upper bound can still win (gains only shrink while covered grows, so the result
 * is the same integers as lazy = 0): per round the stale candidates are refreshed in descending (bound, -j) order, one per
 * wave and pass, until the largest key belongs to a candidate refreshed in this round.  `ub`: the bounds are read at entry and
 * written at exit; INT32_MAX = unknown; the caller promises ub[e, j] >= candidate j's true gain against covered_in, which holds
 * across calls while the env's covered set only grows.  With ub == NULL the bounds are internal.  With gains0 != NULL, ub == NULL
 * or lazy == 0, round 0 evaluates every candidate (one wave each, 16 bytes per lane).  Rounds after the first run in one
 * workgroup per env, whose covered row lives in covered_out.  No global atomics, every output element written once per call,
 * no host synchronisation, no allocation.  Deterministic.
 * Returns hipErrorInvalidValue for n outside 1..65535, k or rounds outside 1..4096, words not a positive multiple of 4, lazy
 * outside 0..1, a NULL mask_bits, choice or gain, rounds > 1 without covered_out, or a mask_bits / covered_in / covered_out
 * that is not 16-byte aligned.  [host struct]; pointers are device. */
typedef struct GnbvCoverGreedy {
    int n, k, words, rounds;        /* envs, candidates per env, words per row, T >= 1 */
    const int32_t *mask_bits;       /* [n, k, words] */
    const int32_t *covered_in;      /* [n, words], or NULL = nothing covered */
    const uint8_t *contact;         /* [n, k], or NULL; != 0: never chosen unless every candidate of the env is */
    int32_t *choice, *gain;         /* [n, rounds] */
    int32_t *covered_out;           /* [n, words] = covered_in | the chosen masks; required when rounds > 1, else may be NULL;
                                     * may alias covered_in */
    int32_t *gains0;                /* [n, k], or NULL: every candidate's gain against covered_in */
    int32_t *ub;                    /* [n, k], or NULL: in/out upper bounds */
    int lazy;                       /* 1 = lazy evaluation, 0 = every candidate in every round; the same results */
} GnbvCoverGreedy;
int gnbv_cover_greedy(const GnbvCoverGreedy *args /*[host]*/, void *stream);

/* Weighted greedy set cover over 1..4 planes of per-candidate bit masks (a new entry point of ABI 5): the set cover whose score
 * is a weighted sum of the planes' gains, against one covered set per plane that grow together.  With plane 0 =
 * gnbv_view_gain_masks' unknown_bits, plane 1 = its hit_bits and weights (w0, w1) the round-0 score is the view-gain score
 * w0 unknown + w1 unknown_hit of every candidate.  Per env, with covered_p = covered_in[p] (NULL: empty), for round
 * t = 0 .. rounds-1:
 *   g_pj = popcount(mask_p[j] & ~covered_p);  s_j = sum over p < planes of weight[p] g_pj;  score_j = contact[j] ? -1 : s_j;
 *   j* = the largest score, ties to the lowest j (all candidates in contact: j* = 0);
 *   choice[t] = j*;  gain[t] = s_j* (also of a contact winner);  plane_gain[t, p] = g_pj*;
 *   covered_p |= mask_p[j*] for every p < planes, a plane of weight 0 included.
 * A candidate may win again with gain 0; all weights 0 is legal (every round: the lowest candidate not in contact, gain 0).
 * gains0[e, j] = s_j of round 0 for every candidate.  Every g_pj only shrinks while covered_p grows and the weights are not
 * negative, so s_j only shrinks: lazy = 1 gives the same integers as lazy = 0, and `ub`, the bounds of s_j, follows
 * gnbv_cover_greedy's contract word for word -- read at entry, written at exit, INT32_MAX = unknown, the caller promises
 * ub[e, j] >= s_j against covered_in, which holds across calls while every covered set only grows.  With gains0 != NULL, or
 * lazy == 0 and ub != NULL, round 0 evaluates every candidate in a wide launch (one wave each, 16 bytes per lane and plane, all
 * planes' rows in one trip).  The rounds run in one workgroup per env, whose covered rows live in covered_out[p]; the winner's
 * plane gains are taken in the pass that ORs its rows into them.  No global
 * atomics, every output element written once per call, no host synchronisation, no allocation.  Deterministic.  planes = 1 with
 * weight 1 gives gnbv_cover_greedy's outputs byte for byte.
 * Returns hipErrorInvalidValue for everything gnbv_cover_greedy refuses (n outside 1..65535, k or rounds outside 1..4096, words
 * not a positive multiple of 4, lazy outside 0..1, a NULL choice or gain), planes outside 1..4, and for p < planes: a negative
 * weight[p], a NULL mask_bits[p], a mask_bits[p] / covered_in[p] / covered_out[p] that is not 16-byte aligned, rounds > 1 with a
 * NULL covered_out[p], a covered_out[p] that is also another plane's covered_out; and for
 * (weight[0] + .. + weight[planes-1]) * 32 * words > INT32_MAX (a score would not fit in int32).  Entries p >= planes are
 * ignored.  [host struct]; pointers are device. */
typedef struct GnbvCoverGreedyW {
    int n, k, words, rounds;        /* as GnbvCoverGreedy */
    int planes;                     /* 1..4 */
    int weight[4];                  /* >= 0 for p < planes */
    const int32_t *mask_bits[4];    /* [n, k, words] each */
    const int32_t *covered_in[4];   /* [n, words] or NULL = nothing covered, per plane */
    int32_t *covered_out[4];        /* [n, words] = covered_in[p] | the chosen rows of plane p; all planes required when
                                     * rounds > 1, else each may be NULL; may alias its own covered_in */
    const uint8_t *contact;         /* [n, k] or NULL; != 0: never chosen unless every candidate of the env is */
    int32_t *choice, *gain;         /* [n, rounds]; gain = the weighted score of the winner */
    int32_t *plane_gain;            /* [n, rounds, planes] or NULL: the winner's true gain per plane */
    int32_t *gains0;                /* [n, k] or NULL: weighted round-0 score of every candidate */
    int32_t *ub;                    /* [n, k] or NULL: in/out upper bounds of the weighted score */
    int lazy;                       /* 1 = lazy evaluation, 0 = every candidate in every round; the same results */
} GnbvCoverGreedyW;
int gnbv_cover_greedy_w(const GnbvCoverGreedyW *args /*[host]*/, void *stream);

/* ------------------------------------------------------------------------- */
/* Plan-then-fly (a new entry point of ABI 5): order a set of points into a    */
/* short open flight tour from a matrix of integer leg lengths.                */
/* ------------------------------------------------------------------------- */
/* Per env, D = dist_mm[e] ([p, p] u32 millimetres, 0xFFFFFFFF = no route; read as given, D[a][b] is the entry of row a, the
 * matrix is assumed symmetric and never checked), c = count[e] (NULL: p):
 *   route set   = {0} and every j in 1 .. c-1 with D[0][j] != 0xFFFFFFFF.  routed = R = its size.  Point 0 is the fixed start,
 *                 the path is open (no return to the start).  Every other index of 0 .. p-1 (j >= c included) goes to
 *                 order[R ..] in ascending order.
 *   construction: t[0] = 0; then R - 1 times the unvisited route point j with the smallest D[t[last]][j] is appended, ties to the
 *                 lowest j.
 *   improvement : best-improvement 2-opt.  A round looks at every 1 <= i < j <= R-1 with, in signed 64 bits,
 *                   delta = D[t[i-1]][t[j]] - D[t[i-1]][t[i]] + (j+1 < R ? D[t[i]][t[j+1]] - D[t[j]][t[j+1]] : 0)
 *                 and takes the most negative delta, ties to the lowest i, then the lowest j.  No delta below 0: done.  Else, if
 *                 max_moves moves have been made already, status bit 2 is set and the loop stops; else t[i .. j] is reversed
 *                 (one move) and the next round starts.  On a symmetric D every move shortens an integer length, so the loop
 *                 ends; max_moves bounds it whatever D holds.
 *   order[0 .. R-1] = t;  length_mm = the sum of D[t[q]][t[q+1]], q = 0 .. R-2, in 64 bits.
 *   status bit 1: some entry the rule reads between two route points was 0xFFFFFFFF -- D[t[last]][j] of every unvisited route
 *                 point j in every construction step, the two or four entries of every pair of every 2-opt round (the round
 *                 that finds nothing and the round that meets the cap included), or a leg of the final route.  Such an entry is
 *                 used as the plain number 4294967295, so the result stays defined.  (On a symmetric D: exactly when two route
 *                 points have no route between them.)
 *   status bit 2: the max_moves cap, as above.
 *   status bit 4: c outside 1 .. p.  The env gets order = 0 .. p-1, routed = 1, length_mm = 0, and no other bit.
 * One workgroup per env, D and the tour in LDS.  Integers with one right answer.  No global atomics, every output element
 * written once per call, no host synchronisation, no allocation.  Deterministic.
 * Returns hipErrorInvalidValue for a NULL struct, n outside 1..65535, p outside 1..128, max_moves < 0, or a NULL dist_mm, order,
 * routed, length_mm or status.  [host struct]; pointers are device. */
typedef struct GnbvTourRoute {
    int n, p;                 /* envs 1..65535, points per env 1..128 */
    const uint32_t *dist_mm;  /* [n,p,p], 0xFFFFFFFF = no route; read as given, assumed symmetric */
    const int32_t *count;     /* [n] or NULL (= p) */
    int max_moves;            /* >= 0 */
    int32_t *order;           /* [n,p] */
    int32_t *routed;          /* [n] */
    int64_t *length_mm;       /* [n] */
    int32_t *status;          /* [n] */
} GnbvTourRoute;
int gnbv_tour_route(const GnbvTourRoute *args /*[host]*/, void *stream);

/* ------------------------------------------------------------------------- */
/* Depth sensor model: what a real depth camera would have returned for a      */
/* frame of gnbv_render_depth -- range limits, dropouts at depth edges and at  */
/* random, range noise, disparity quantisation (a new entry point of ABI 5).   */
/* ------------------------------------------------------------------------- */
/* Input frame depth_in / seg_in: f32 [n, h, w] as gnbv_render_depth writes them, rows contiguous, env e at base + e in_env_stride
 * (in floats, >= h w); output frame depth_out / seg_out the same with out_env_stride.  r is the raw value and t = -r.
 * GNBV_DEPTH_NO_RETURN (below) is the raw depth of a pixel the sensor got no return for.
 * Every fp32 operation is the correctly rounded one (fadd, fsub, fmul, fdiv = the _rn intrinsics), in the order given.
 *
 * Class of an input pixel, from the input alone:
 *   MISS  r == -inf;
 *   RET   t finite and min_range <= t <= max_range;
 *   FAR   t finite and t > max_range;
 *   VOID  everything else: NaN, +inf, t <= 0, t < min_range.
 * MISS and FAR give (-inf, 0.0f); VOID gives (GNBV_DEPTH_NO_RETURN, 0.0f).  A RET pixel p = (e, v, u), in this order:
 *   1. (w0, w1, w2, w3) = Philox4x32-10 of the counter (v w + u, e, frame[e], 0) under the key (seed & 0xffffffff, seed >> 32);
 *      frame is int32 [n] on the device, read and never written.  All four words are drawn whichever effects are enabled.
 *   2. edge test, skipped when edge_radius == 0: thr = fadd(edge_abs, fmul(edge_rel, t_p)); p is an EDGE pixel iff some q != p of
 *      the (2 edge_radius + 1)^2 window around p, inside the image, is not RET, or is RET with fabsf(fsub(t_q, t_p)) > thr
 *      (neighbours outside the image are ignored).  An edge pixel is dropped iff edge_drop == 0xFFFFFFFF, or edge_drop != 0 and
 *      w0 < edge_drop.
 *   3. random dropout: the pixel is dropped iff drop == 0xFFFFFFFF, or drop != 0 and w1 < drop.
 *   4. range noise: z = gauss_lut[w2 >> 20] (the caller's table of 4096 floats on the device; 0 where it is NULL);
 *      sigma = fadd(fadd(sigma0, fmul(sigma1, t)), fmul(sigma2, fmul(t, t)));  t1 = fadd(t, fmul(sigma, z)).
 *   5. disparity quantisation: t2 = quant > 0 ? fdiv(quant, rintf(fdiv(quant, t1))) : t1 (rintf rounds ties to even).
 *   6. a dropped pixel gives (GNBV_DEPTH_NO_RETURN, 0); else !(t2 >= min_range) gives (GNBV_DEPTH_NO_RETURN, 0); else
 *      t2 > max_range (+inf from a zero divisor included) gives (-inf, 0); else (-t2, seg_in[p]) with the seg bits copied.
 * The result is a pure function of (the inputs, seed, frame[e], e, v, u): it depends neither on n, nor on the launch shape, nor
 * on what other envs hold.
 *
 * Why the no-return value is a tiny negative number and not NaN or 0: under the measured-frame rule of gnbv_view_gain above, NaN,
 * +-0 and -inf are RANGE-ENDED, so a carve would free a dropped pixel's ray all the way to the sensor's range, straight through
 * whatever the sensor failed to see.  -2^-100 is finite, non-zero and above the clamp: SURFACE-ENDED with length 2^-100, its
 * target voxel the camera's own, so the ray marks and carves nothing; with seg 0 the pixel is not foreground, so the voxel
 * update and the scan set ignore it.
 *
 * One launch on the caller's stream; no workspace, no allocation, no host synchronisation, no atomics.  Every output element of
 * every env's h w block is written; bytes between the blocks are not touched.
 * Returns hipErrorInvalidValue, before any launch, for: a NULL struct; n, h or w < 1; h w > 2^32 - 1; an env stride below h w; a
 * NULL depth_in, seg_in, depth_out, seg_out or frame; gauss_lut NULL with a sigma above 0; any overlap of an output span
 * [base, base + (n - 1) stride + h w) with an input span or of the two output spans (the stencil reads neighbours: in place is
 * refused); and any parameter outside the ranges noted in the struct.  [host struct]; pointers are device. */
#define GNBV_DEPTH_NO_RETURN (-0x1p-100f)
typedef struct GnbvDepthSensor {
    int n, h, w;
    const float *depth_in, *seg_in;
    int64_t in_env_stride;
    float *depth_out, *seg_out;
    int64_t out_env_stride;
    const int32_t *frame;            /* [n] device */
    uint64_t seed;
    float min_range, max_range;      /* 0 < min_range <= max_range, finite */
    int edge_radius;                 /* 0..2 */
    float edge_abs, edge_rel;        /* >= 0, finite */
    uint32_t edge_drop, drop;        /* thresholds on a 32-bit word: 0 never, 0xFFFFFFFF always */
    float sigma0, sigma1, sigma2;    /* >= 0, finite */
    const float *gauss_lut;          /* [4096] device; may be NULL iff all three sigmas are 0 */
    float quant;                     /* >= 0, finite; 0 = off */
} GnbvDepthSensor;
int gnbv_depth_sensor(const GnbvDepthSensor *args /*[host]*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GENNBV_HIP_H */
