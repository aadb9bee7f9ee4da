/*
 * ppp_hip.h -- C ABI of the MI355X (gfx950) polishing-path engine.
 *
 * This is the drop-in boundary: the reference's planner classes
 * (include/Path_Generate.h, include/Path_Generate_Algorithm.h,
 * include/robot_path.h of tsai0507/PolishPathPlanning) keep their public
 * methods and forward the arithmetic to these entry points; see
 * INTEGRATION.md for the binding a maintainer adds.  Plain C types only, an
 * opaque handle, caller-allocated outputs (two-call size query: pass cap = 0
 * to learn the count), `int` status everywhere (0 = ok, < 0 = error; nothing
 * throws or aborts across the boundary).  One handle = one device + one HIP
 * stream; distinct handles may be used from distinct threads.
 *
 * Each entry point cites the reference code it replaces (file:line relative
 * to the reference tree).
 */
#ifndef PPP_HIP_H
#define PPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ppp_handle_s *ppp_handle;

/* status codes */
enum {
    PPP_OK = 0,
    PPP_ERR_ARG = -1,          /* bad argument / call order                                  */
    PPP_ERR_HIP = -2,          /* a HIP runtime call failed (ppp_last_error has the text)     */
    PPP_ERR_NO_DEVICE = -3,    /* no gfx950 device: the engine has no CPU fallback            */
    PPP_ERR_SLICE = -4,        /* a slice has an empty side or < 3 nodes: the reference aborts
                                  there; ppp_failed_slice() names it     */
    PPP_ERR_CAPACITY = -5,     /* an internal capacity was exceeded (reported, never silent)  */
    PPP_ERR_DOMAIN = -6,       /* spline evaluated outside [miny, bigy] (GSL_EDOM)            */
    PPP_ERR_UNSUPPORTED = -7,  /* option outside the hot-path scope (e.g. Alignment=true)     */
    PPP_ERR_IO = -8
};

/* insert_point flavour */
enum { PPP_PAIR_KD = 0,      /* src/Path_Alg/path_slicing_alg.cpp:164-237 (connect, connect1, contour) */
       PPP_PAIR_BRUTE = 1    /* src/Path_Generation.cpp:107-206 (./main)                                */ };

/* slice-position walk */
enum { PPP_WALK_SECTPATH = 0,   /* SectPath::GenPath, path_slicing_alg.cpp:308-330        */
       PPP_WALK_CENTER_INT = 1, /* path_generater::GenPath + thread_worker,
                                   path_dynamic_alg.cpp:308-372 (connect)                  */
       PPP_WALK_SDIR_INT = 2,   /* dynamic_alg_sdir.cpp:349-374 (connect1)                */
       PPP_WALK_V1_CONTACT = 3, /* Contact_Path_Generation, Path_Generation.cpp:711-725   */
       PPP_WALK_V1_SLICING = 4  /* slicing_method, Path_Generation.cpp:295-304            */ };

/* All config.txt keys (config.txt:1-13) + the compile-time constants of the reference. */
typedef struct ppp_params {
    double tool_radius;       /* Tool_Radius                                                  */
    double path_resolution;   /* PathResolution                                               */
    double rpy_resolution;    /* RPYresolution                                                */
    float  ee_length;         /* End effector length (m)                                      */
    int    change_range;      /* ChangeRange                                                  */
    int    pairing;           /* PPP_PAIR_*                                                   */
    int    walk;              /* PPP_WALK_*                                                   */
    double trim;              /* 10: path_translation_alg.cpp:158-159; 5: contour_alg.cpp:496 */
    int    drop_ends;         /* 1: path_translation_alg.cpp:149-150                          */
    int    smooth;            /* 1: postion_smooth() applied (path_translation_alg.cpp:212)   */
    float  handeye[6];        /* HANDEYEx..rz (Path_Generate_Algorithm.h:43-48)               */
    float  normal_radius;     /* 2.5 (path_slicing_alg.cpp:147)                               */
    int    smooth_max_sweeps; /* unused by the engine (postion_smooth is solved directly, ppp_kernels.h a13); the
                                 oracle's sequential sweep takes it as its cap     */
    int    alignment;         /* must be 0: Alignment / Smooth / RemoveOutlier are the ppp_trans2center / ppp_smooth_mls / ppp_remove_outlier calls */
    int    dynamic_adjustment;/* Dynamic_adjustment (config.txt:13): path_dynamic_alg.cpp:77-306 for the connect /
                                 connect1 walks, Path_Generation.cpp:362-634 for PPP_WALK_V1_CONTACT            */
    double depth;             /* depth            (config.txt:5)                              */
    double adjust_threshold;  /* Adjust_Threshold (config.txt:3)                              */
    double toolthickness;     /* toolthickness    (config.txt:4)                              */
    int    curvature_k;       /* neighbours of compute_transform: 50 (path_dynamic_alg.cpp:87) */
    /* Slice-range sharding of ONE cloud over several GPUs (SURVEY.md 8e case ii): this handle plans the slices
       [slice_begin, slice_end) of the walk only (slice_end <= 0: up to the last one).  Every handle still takes the
       whole cloud (the walk needs its bounds) but indexes only the points within range_margin mm of its slices.
       getPath then stops after HandEyeTransform (a12): postion_smooth couples neighbouring slices
       (path_translation_alg.cpp:117-140), so it runs once on the gathered list -- ppp_finish_path_async. */
    int    slice_begin, slice_end;
    float  range_margin;      /* mm kept beyond the first/last band of the range (default 24) */
} ppp_params;

void ppp_default_params(ppp_params *p);

/* ---- lifetime ---- */
int ppp_create(int device_id, ppp_handle *out);
int ppp_destroy(ppp_handle h);
const char *ppp_last_error(ppp_handle h);
const char *ppp_version(void);

int ppp_set_params(ppp_handle h, const ppp_params *p);

/* Replaces the constructors' load + scale loop (path_slicing_alg.cpp:10-25,
 * Path_Generation.cpp:8-34, path_dynamic_alg.cpp:12-28): takes the points as read from
 * the PCD (xyz every `stride_bytes`: 32 = pcl::PointXYZRGB, 16, or 12 packed), applies
 * the x1000 when change_range is set, keeps the cloud resident in HBM.
 * viewpoint = PCD VIEWPOINT translation (cloud.sensor_origin_), NULL = origin. */
int ppp_set_cloud(ppp_handle h, const float *xyz_host, size_t n, size_t stride_bytes, const float *viewpoint);
/* same, the buffer already lives on this handle's device */
int ppp_set_cloud_device(ppp_handle h, const float *xyz_dev, size_t n, size_t stride_bytes, const float *viewpoint);
/* same, without waiting for the conversion pass where the handle can do without (see ppp_set_plan_reuse: it holds a window plan
 * of an earlier cloud of this size and these parameters): returns as soon as that pass is enqueued on the handle's stream, and a
 * pass of the new cloud may be enqueued right behind it.  xyz_dev must stay as it is until a call that waits has returned
 * (ppp_sync, any getter) -- or, for a caller that orders its own work after the handle's stream (ppp_get_stream), until that
 * stream has passed this point.  Where the handle cannot do without the bounds this is ppp_set_cloud_device. */
int ppp_set_cloud_device_async(ppp_handle h, const float *xyz_dev, size_t n, size_t stride_bytes, const float *viewpoint);
/* The constructors' first line and their loop in one call (pcl::io::loadPCDFile<PointXYZRGB>(name, *cloud) + the x1000 loop:
 * path_slicing_alg.cpp:10-25, path_dynamic_alg.cpp:12-28, Path_Generation.cpp:8-34): the file's records go straight to HBM.
 * A `DATA binary` file whose x, y, z are consecutive float32 fields is streamed in pieces through two pinned buffers that
 * belong to the handle (several readers fill one while the other is on its way to the device; the conversion kernel then picks
 * x, y, z out of the records: no host copy of the cloud is ever made); every other flavour (ascii, binary_compressed, F8
 * or integer coordinates) goes through ppp_load_pcd + ppp_set_cloud.  *n = the points of the file, viewpoint_out (7 floats,
 * may be NULL) its VIEWPOINT line; the translation part becomes the handle's viewpoint as in ppp_set_cloud. */
int ppp_set_cloud_pcd(ppp_handle h, const char *path, size_t *n, float viewpoint_out[7]);
/* Slice-range sharding without the whole cloud on every GPU (SURVEY.md 8e case ii, pre-partitioned by x).
 * ppp_range_interval: the x interval [lo, hi] -- planner units: the file's values x 1000 (as floats) when ChangeRange -- whose
 * points a handle with p->slice_begin / slice_end / range_margin indexes, for a cloud with the given x bounds (host arithmetic
 * only: the slice walk of path_slicing_alg.cpp:308-330 etc.; +-INFINITY for the whole walk, lo > hi for an empty range);
 * *num_slices (optional) receives S.
 * ppp_set_cloud_part: like ppp_set_cloud, but xyz holds only the n_part points of the cloud whose planner-unit x lies in
 * [part_lo, part_hi], in the cloud's own order (index ties then break as in the whole cloud); cloud_index (optional) = their
 * indices in the whole cloud, so that every index the engine reports is the cloud's; mn / mx / n_valid_total = pcl::getMinMax3D
 * and the number of finite points of the WHOLE cloud in planner units (ranks agree on them with one all-reduce of 3 minima,
 * 3 maxima and a count).  The handle must be given a slice range whose interval lies inside [part_lo, part_hi]; it then plans
 * exactly what a whole-cloud handle with that range plans (same slab grid, bit-identical list).  Calls that address points by
 * whole-cloud index or replace the cloud (ppp_insert_point, ppp_normals_at, ppp_estimate_normals, the preprocessing) are refused. */
int ppp_range_interval(const ppp_params *p, float min_x, float max_x, float *lo, float *hi, int *num_slices);
int ppp_set_cloud_part(ppp_handle h, const float *xyz_host, size_t n_part, size_t stride_bytes, const float *viewpoint,
                       const int *cloud_index, const float mn[3], const float mx[3], size_t n_valid_total, float part_lo, float part_hi);
int ppp_num_points(ppp_handle h, size_t *n);
/* the resident cloud (after the x1000 and any preprocessing) as n x 3 packed floats in index order */
int ppp_get_cloud(ppp_handle h, float *xyz, size_t cap, size_t *n);

/* ---- the nominal part as a triangle mesh (a CAD export): sampled on the device into the resident cloud ----
 * ppp_set_cloud_mesh puts a deterministic sampling of the mesh's surface on the handle; from then on the handle is what
 * ppp_set_cloud leaves for a cloud whose conversion yields exactly those floats (plan, bounds, viewpoint, caches; a handle with a
 * slice range indexes its part of the samples; ppp_get_cloud returns them, with no second x1000), so every call that takes a
 * cloud -- ppp_get_deviation and the registrations with this handle as `ref`, their tiles, the contact field, a plan on the
 * nominal itself -- works on it unchanged.
 * verts = n_verts x 3 packed floats in the file's units; tris = n_tris x 3 vertex indices, or NULL for a soup (triangle f uses
 * vertices 3f, 3f + 1, 3f + 2; n_verts must be 3 n_tris).  Every vertex goes through ppp_set_cloud's conversion (the x1000 when
 * change_range is set, non-finite -> NaN); the rule below works on those floats widened to double, with + - * /, sqrt and ceil,
 * one rounding per written operation.  pitch is in resident units (mm after ChangeRange).  Per triangle (a, b, c):
 *   squared edge lengths ab, bc, ca, each (dx dx + dy dy) + dz dz; rotate cyclically (the winding stays) so that the longest
 *   edge is (p0, p1) and p2 lies opposite, a tie going to the first of ab, bc, ca; e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2,
 *   A2 = sqrt((nx nx + ny ny) + nz nz), L = sqrt(longest), hgt = A2 / L;
 *   degenerate: an index outside [0, n_verts), a coordinate that is not finite, A2 zero or not finite -- skipped and counted;
 *   PPP_MESH_FRONT: culled -- skipped and counted -- unless ((nx (vx - p0x) + ny (vy - p0y)) + nz (vz - p0z)) > 0, v = viewpoint
 *   (NULL = origin) in the frame and units in which ppp_estimate_normals orients normals: resident ones.  It trusts the winding;
 *   rows R = max(1, ceil(hgt / pitch)); row r: t = (r + 0.5) / R, len = L (1 - t), M_r = max(1, ceil(len / pitch));
 *   column k of row r: s = (k + 0.5) / M_r, w = s (1 - t); the sample is (p0 + e2 t) + e1 w per coordinate, rounded to float.
 * Samples are ordered by triangle, row, column: the cloud's index order.  Each lies strictly inside its triangle; the density
 * is about 1 / pitch^2 whatever the triangle's shape (rows run along the longest edge: a sliver 50 long and 0.05 high is one row).
 * tri_index (optional): the triangle of sample i, the first min(cap, samples) entries.  stats (optional) is filled as far as the
 * counts were reached: triangles = n_tris = sampled + degenerate + culled; rows and samples are the totals.
 * PPP_ERR_ARG: NULL verts or mp, pitch not > 0 or not finite, unknown facing, a soup with n_verts != 3 n_tris, n_tris == 0, no
 * sample at all (every triangle degenerate or culled); PPP_ERR_CAPACITY: more rows or samples than a resident cloud holds
 * ((2^31 - 1) / 8 points, as ppp_set_cloud); PPP_ERR_UNSUPPORTED: the handle holds a part (ppp_set_cloud_part).  A refused call
 * leaves the resident cloud and the plan as they were.
 * Not here: the handle's normals stay the PCA normals of its samples (not the facets'), and vertices are not welded.  A point is
 * measured against the triangles themselves by ppp_trimesh_nearest and ppp_get_mesh_deviation, further down.
 * ppp_set_cloud_stl: ppp_load_stl + ppp_set_cloud_mesh of the soup; PPP_ERR_IO for a file that cannot be read. */
enum { PPP_MESH_ALL = 0, PPP_MESH_FRONT = 1 };
typedef struct { float pitch; int facing; } ppp_mesh_params;      /* defaults 0.5, PPP_MESH_ALL */
typedef struct { size_t triangles, sampled, degenerate, culled, rows, samples; } ppp_mesh_stats;
void ppp_default_mesh_params(ppp_mesh_params *mp);
int  ppp_set_cloud_mesh(ppp_handle h, const float *verts, size_t n_verts, const int *tris, size_t n_tris,
                        const ppp_mesh_params *mp, const float *viewpoint,
                        int *tri_index, size_t cap, ppp_mesh_stats *stats);
int  ppp_set_cloud_stl(ppp_handle h, const char *path, const ppp_mesh_params *mp, const float *viewpoint,
                       ppp_mesh_stats *stats);

/* ---- preprocessing of the constructors, on the resident cloud ---- */
/* SectPath::remove_outlier() (path_slicing_alg.cpp:101-108): pcl::StatisticalOutlierRemoval, setMeanK(mean_k = 50),
 * setStddevMulThresh(stddev_mul = 1.0), sor.filter(*cloud): the filtered cloud replaces the resident one (same order,
 * new indices), the plan is rebuilt.  n_kept / threshold (mean + mul * stddev of the per-point mean neighbour
 * distances) are optional outputs.  mean_k <= 63. */
int ppp_remove_outlier(ppp_handle h, int mean_k, double stddev_mul, size_t *n_kept, double *threshold);
/* path_generater::voxel_down(x, y, z) (Path_Generation.cpp:53-59): pcl::VoxelGrid, setLeafSize(x, y, z), sor.filter(*cloud)
 * with the class defaults: one point per occupied voxel (float centroid of its points), in ascending voxel id; replaces
 * the resident cloud, the plan is rebuilt.  Leaf sizes in the cloud's units (mm after ChangeRange).  *overflow = 1 and
 * the cloud is left as it is where PCL warns "Leaf size is too small ... Integer indices would overflow". */
int ppp_voxel_down(ppp_handle h, float leaf_x, float leaf_y, float leaf_z, size_t *n_out, int *overflow);
/* SectPath::trans2center() (path_slicing_alg.cpp:82-99; v1 Path_Generation.cpp:60-92): centroid and covariance as
 * pcl::compute3DCentroid / pcl::computeCovarianceMatrix accumulate them (float, point after point -- reproduced bit for
 * bit on the device), Eigen::EigenSolver<Matrix3f> eigenvectors (unsorted, as they come), TransAlign = [V^T | -V^T c],
 * pcl::transformPointCloud on the resident cloud.  From then on ppp_get_path applies invTransAlign to the sampled
 * points and looks up the nearest point and its normal in the cloud carried back by the inverse
 * (path_translation_alg.cpp:146-174), until ppp_set_cloud.  Optional outputs: TransAlign (row-major 4 x 4), the
 * centroid, the 3 x 3 accumulated covariance.  PPP_ERR_DOMAIN when the float Schur form keeps a complex pair. */
int ppp_trans2center(ppp_handle h, float *trans_align16, float *centroid3, float *covariance9);
/* SectPath::smooth() (path_slicing_alg.cpp:111-139; v1 Path_Generation.cpp:340-360): pcl::MovingLeastSquares with
 * setPolynomialOrder(order = 3), setSearchRadius(search_radius = 15), SIMPLE projection, no upsampling; the projected
 * points replace the resident cloud (points with fewer than 3 neighbours in the radius, and non-finite points, are
 * not in the output), the plan is rebuilt.  Radius in the cloud's units (mm after ChangeRange); order 0..3 (0 and 1:
 * projection on the local plane only).  The "smooth_<name>" PCD side file of the reference is the caller's to write. */
int ppp_smooth_mls(ppp_handle h, double search_radius, int order, size_t *n_out);

/* ---- whole hot path, asynchronous on the handle's stream ---- */
/* GenPath(): getMinMax3D + slice walk + rangedX_index + insert_point + Spline for every
 * slice (path_slicing_alg.cpp:290-342, path_dynamic_alg.cpp:337-372 with Adjust=false,
 * Path_Generation.cpp:282-304,659-727 without the dynamic adjustment). */
int ppp_gen_path_async(ppp_handle h);
/* getPath(): path_translation_alg.cpp:144-214 (sampling, normals, pose, HandEye, smoothing,
 * reduceRPY, TransFlangeposition); the list stays in HBM. */
int ppp_get_path_async(ppp_handle h);
/* GenPath() followed by getPath() as ONE enqueue: the kernel sequence is captured into a hipGraph
 * the first time and replayed afterwards (one host call per workpiece instead of ~10 launches;
 * this is what keeps a batch of small workpieces from being host-launch-bound).  Falls back to
 * the two plain calls while kernel timing is enabled. */
int ppp_run_async(ppp_handle h);
/* Batched form (SURVEY.md 8b / BASELINE config 3: many small workpieces on ONE GPU): GenPath + getPath of
 * `count` handles of the same device as ONE hipGraph whose branches (one per handle) run side by side --
 * one host call per batch instead of one per workpiece.  When dst_dev is not NULL every branch's last
 * kernel also writes its WayPointsList to dst_dev + 6 * offset_rows[i] (at most cap_rows[i] rows; a longer
 * list is an error of that handle), so the batch lands in one caller-owned device buffer (the RCCL send
 * buffer) without a host round trip.  Graphs are cached in hs[0] (two: a caller may alternate between two
 * destinations) and rebuilt when the handle list, a handle's plan or the destination changes.  Follow with
 * ppp_sync_batch (or any per-handle call, which waits). */
int ppp_run_batch_async(ppp_handle *hs, size_t count, float *dst_dev, const size_t *offset_rows, const size_t *cap_rows);
/* waits for the batch, returns the first handle's error (index in *failed when not NULL) */
int ppp_sync_batch(ppp_handle *hs, size_t count, size_t *failed);
/* Multi-GPU exchange of the finished lists: variable-length gather to `root` over RCCL.  Rank r
 * contributes the counts_rows[r] rows of its WayPointsList; on root, recv_dev (device memory, sum(counts) x 6 floats)
 * receives the blocks back to back in rank order.  One ncclGroup of direct ncclSend / ncclRecv pairs -- point to point
 * over xGMI, no ring -- on the handle's stream (asynchronous; ppp_sync afterwards).  nccl_comm is the caller's
 * ncclComm_t (one rank per process / GPU); librccl is looked up at the first call (dlopen), the engine itself does not
 * link it.  Frameworks that own the communicator (torch.distributed) use their own collective on the list's device
 * pointer instead -- polishpathplanning_amd/robot_path.py.
 * nranks == 1: with nccl_comm == NULL the list is copied to recv_dev; with a (one-rank) communicator it goes through librccl's
 * group -- ncclSend to self + ncclRecv from self -- which is the pre-flight of this exchange on one GPU. */
int ppp_gather_waypoints(ppp_handle h, void *nccl_comm, int rank, int nranks, int root, const size_t *counts_rows, float *recv_dev);
/* the handle's HIP stream (hipStream_t), so a framework can order its own work after the planner's on the GPU
 * (e.g. torch.cuda.ExternalStream + wait_stream before the RCCL gather) instead of waiting on the host */
int ppp_get_stream(ppp_handle h, void **stream);
/* waits for the stream, then reports deferred device-side errors */
int ppp_sync(ppp_handle h);
int ppp_failed_slice(ppp_handle h);

/* ---- results (each call synchronises the handle's stream) ---- */
int ppp_num_slices(ppp_handle h, int *S);
int ppp_num_waypoints(ppp_handle h, size_t *W);
/* WayPointsList: W x 6 floats (x y z roll pitch yaw), what getPath writes to pathFile
 * (path_translation_alg.cpp:216-228) */
int ppp_get_waypoints(ppp_handle h, float *out6, size_t cap, size_t *W);
/* device pointer of the same list (valid until the next ppp_get_path_async / destroy) */
int ppp_get_waypoints_device(ppp_handle h, const float **dptr, size_t *W);
/* copies the list into a caller-owned DEVICE buffer (e.g. a framework tensor used as the
 * send buffer of the RCCL gather); asynchronous on the handle's stream after the count is known */
int ppp_copy_waypoints_to_device(ppp_handle h, float *dst_dev, size_t cap, size_t *W);
/* waypoints of every kept slice in list order (the sizes of the reference's per-slice vectors,
 * path_translation_alg.cpp:156-169); zero for slices outside this handle's slice range */
int ppp_get_waypoint_counts(ppp_handle h, int *counts, size_t cap, size_t *nkept);
/* copies a W x 6 stage list (PPP_STAGE_WP_PRESMOOTH / PPP_STAGE_WP_SMOOTHED) into a caller-owned DEVICE buffer */
int ppp_copy_stage_to_device(ppp_handle h, int stage, float *dst_dev, size_t cap, size_t *W);
/* Second half of getPath on a list assembled elsewhere: postion_smooth, reduceRPY, TransFlangeposition
 * (path_translation_alg.cpp:212-214) over `W` pre-smoothing waypoints in DEVICE memory (the blocks of
 * the slice-range handles concatenated in slice order) with `counts[nkept]` waypoints per kept slice.
 * Needs a handle planned for the same cloud and parameters (any slice range).  The result is read
 * with ppp_get_waypoints / ppp_copy_waypoints_to_device / ppp_get_tail_index as after getPath. */
int ppp_finish_path_async(ppp_handle h, const float *pre6_dev, size_t W, const int *counts, size_t nkept);
/* TailIndex (path_translation_alg.cpp:177,210) */
int ppp_get_tail_index(ppp_handle h, int *tail, size_t cap, size_t *n);

/* pcl::getMinMax3D (path_slicing_alg.cpp:303) */
int ppp_minmax(ppp_handle h, float mn[3], float mx[3]);
/* plane x of every slice in Path_set order */
int ppp_get_slice_positions(ppp_handle h, float *px, size_t cap, size_t *S);
/* rangedX_index result of slice s, ascending cloud indices */
int ppp_get_slice_indices(ppp_handle h, int s, int *out, size_t cap, size_t *n);
/* Spline knots of slice s (ascending y): what OnePath / path_track feed to Spline() */
int ppp_get_nodes(ppp_handle h, int s, double *y, double *x, double *z, size_t cap, size_t *m);
/* Dynamic adjustment only: the boundary spline slice s was adjusted against -- compute_boundary(pre_path, boundary, key) of
   thread_worker (path_dynamic_alg.cpp:183-235, 320-322; v1: Path_Generation.cpp:585-592), the curve drawpath(*boundary, 0,255,0)
   paints: knots in ascending y with the two end knots 20 mm out.  *m = 0 where compute_boundary returned 0 at that step (fewer than
   3 boundary points: nothing is painted, the slice is adjusted against the chain's previous boundary) and for the slice a chain starts
   from.  *step = the slice's step in its chain (0 = next to the start slice; -1 = the start slice itself, or no dynamic adjustment):
   the order thread_worker adjusts -- and paints -- in.  Evaluate with ppp_spline_create / ppp_spline_eval below. */
int ppp_get_boundary(ppp_handle h, int s, double *y, double *x, double *z, size_t cap, size_t *m, int *step);
/* Coverage of the last pass: path_generater::compute_coverage / get_coverage (Path_Generation.cpp:463-467, 483-496, 757-771).
   Every Area2Cloud(point, 1, 0) of compute_boundary (:508-520) -- on every slice's raw path (:719) and, inside dynamic_adjust_path,
   on the adjusted paths of slices 1 .. S-2 (:590) -- marks the cloud points within |min x - max x| / 2 of the point (float
   arithmetic, squared as PCL does).  flags[i] = 1 for a covered cloud point i, 0 otherwise, for the first
   min(cap, *n) points of the cloud; flags may be NULL (the counts only).  *n = cloud->size(), *covered = the yes count.
   get_coverage() prints yes = covered, no = n - covered.  Ordered behind the handle's last pass; blocks until the results are on
   the host.  The first call computes, later calls reuse the result until the next pass or cloud.  PPP_ERR_UNSUPPORTED unless the
   last pass was PPP_WALK_V1_CONTACT with dynamic_adjustment = 1 on a whole-cloud handle (the only flow the reference computes
   coverage in); PPP_ERR_ARG before any pass; the pass's own error if it failed. */
int ppp_get_coverage(ppp_handle h, unsigned char *flags, size_t cap, size_t *n, size_t *covered);
/* Path coverage of the last pass: the contact model of path_generater::compute_coverage / get_coverage (Path_Generation.cpp:
   463-467, 483-496, 757-771) applied to the paths the pass ends with, for every walk.  For every slice
   s of the pass, its final knots (adjusted where the dynamic adjustment ran) and the Steffen spline through them are sampled as
   compute_boundary does (:508-520: dy = miny + 2, step Tool_Radius / 4, while dy < maxy - 2); each sample evaluates Area2Cloud
   with curvature_k, depth, toolthickness and tool_radius, and marks the cloud points within r = (min x - max x) / 2 of it
   (float, r * r compared with the squared distance as PCL does; a NaN r marks nothing).  This is the path set as GenPath
   leaves it: getPath's first / last slice drop and its trim are not applied.  After a PPP_WALK_V1_CONTACT pass with the dynamic
   adjustment it differs from ppp_get_coverage, which also counts the raw paths.
   flags[i] = 1 for a covered cloud point i, 0 otherwise, for the first min(cap, *n) points; flags may be NULL (the counts only).
   *n = cloud->size(), *covered = the yes count.  A slice-range handle marks the balls of its own slices, indexed by whole-cloud
   point index (OR-ing the flags of ranges that tile the walk gives the whole cloud's); PPP_ERR_CAPACITY when one of its searches
   would leave the indexed interval (raise range_margin).  The first call after a pass builds what the pass did not (slab
   index, normal field; a window-path handle stays on the window path) and computes; later calls reuse the result until the
   next pass or cloud.  Blocks until the results are on the host.  PPP_ERR_ARG before any pass or with curvature_k outside
   [3, 64]; PPP_ERR_UNSUPPORTED on a part handle (ppp_set_cloud_part); the pass's own error if it failed. */
int ppp_get_path_coverage(ppp_handle h, unsigned char *flags, size_t cap, size_t *n, size_t *covered);
/* Contact counts of the last pass's paths: the balls of ppp_get_path_coverage, counted.  counts[i] =
   the number of compute_boundary samples whose ball holds cloud point i (at a constant feed, proportional to the tool's dwell
   there); first_slice[i] / last_slice[i] = the smallest / largest slice index with such a ball, -1 where there is none
   (last > first: the band where neighbouring passes overlap).  counts[i] > 0 exactly where ppp_get_path_coverage flags i.
   Each map may be NULL; min(cap, n) entries of each given one are copied.  stats (may be NULL): n = cloud->size(), covered =
   points with a count, multi_slice = points with last > first, max_count, total = the sum of the counts, hist[c] = points
   with count c (hist[PPP_CONTACT_BINS - 1]: count >= PPP_CONTACT_BINS - 1).  A slice-range handle counts the balls of its own
   slices, by global slice index and whole-cloud point index: the counts of ranges that tile the walk add up to the whole
   cloud's, first / last are the minimum / maximum over the ranges that touch a point.  Builds, reuses and refuses as
   ppp_get_path_coverage does, with the same codes, and leaves that call's result alone. */
#define PPP_CONTACT_BINS 64
typedef struct {
    size_t n, covered, multi_slice;
    unsigned int max_count;
    unsigned long long total;
    size_t hist[PPP_CONTACT_BINS];
} ppp_contact_stats;
int ppp_get_path_contacts(ppp_handle h, unsigned int *counts, int *first_slice, int *last_slice, size_t cap,
                          ppp_contact_stats *stats);
/* Predicted material removal of the last pass's paths: the balls of ppp_get_path_contacts -- the same
   slices, samples and float test dist2 <= r2 -- each weighted instead of counted.  A sample stands for the path length
   ds = half the segment to the sample before it plus half the one to the sample after it on its slice (double, from the float
   sample positions; an end sample has one segment, a lone sample none; a segment with a non-finite end is 0), and a held point
   at squared distance d2 inside a ball of squared radius r2 weighs, with u = (double)d2 / (double)r2 (0 when r2 == 0):
     PPP_REMOVAL_FLAT       w = 1            (dwell alone)
     PPP_REMOVAL_PARABOLIC  w = 1 - u
     PPP_REMOVAL_HERTZ      w = sqrt(1 - u)  (the Hertzian pressure profile of a sphere on a surface)
   removal[i] = the sum of w * ds over the balls that hold cloud point i, one double accumulator adding in ascending (slice,
   sample) order: the same bits in every run; 0 for a point no ball holds.  The unit is millimetres of weighted tool travel:
   Preston's constant, the peak pressure, the surface speed and the feed are the caller's factor.  min(cap, n) entries are
   copied; removal may be NULL, stats may be NULL, cap = 0 asks for the statistics alone.  stats: n = cloud->size(), touched =
   points held by at least one ball (ppp_get_path_contacts's covered, whatever the weights), min_removal / max_removal over
   the touched points (NaN when there are none), sum / sum_sq over the touched points by a fixed-order reduction (the same in
   every run), path_length = the sum of every ds of the handle's slices in (slice, sample) order, hist[b] = touched points
   with min(63, floor(removal / max_removal * 63)) == b (all in bin 0 when max_removal == 0).  A slice-range handle sums the
   balls of its own slices by whole-cloud point index: over ranges that tile the walk the maps and the path lengths add up to
   the whole cloud's to within rounding (the association differs, so not bit for bit).  Kept per (pass, profile): a repeated
   call launches nothing.  Builds, reuses and refuses as ppp_get_path_contacts does, with the same codes, shares that call's
   sample table where the handle holds one for the pass, and leaves the results of the other contact calls alone;
   PPP_ERR_ARG for an unknown profile. */
enum { PPP_REMOVAL_FLAT = 0, PPP_REMOVAL_PARABOLIC = 1, PPP_REMOVAL_HERTZ = 2 };
typedef struct {
    size_t n, touched;
    double min_removal, max_removal, sum, sum_sq, path_length;
    size_t hist[PPP_CONTACT_BINS];
} ppp_removal_stats;
int ppp_get_path_removal(ppp_handle h, int profile, double *removal, size_t cap, ppp_removal_stats *stats);
/* A dwell schedule for the last pass's paths: a factor t_j per row j of the sample table of
   ppp_get_path_contacts -- how many times longer than planned the tool stays on the stretch ds_j of sample j -- that steers the
   predicted removal R_i = sum_j a_ij (ds_j t_j) (a_ij: the profile's weight of ppp_get_path_removal for a held pair) towards a
   target map T.  target: n doubles by cloud index, finite and >= 0 at every touched point, or NULL for "uniform, same total":
   T_i = L.  L (stats->level) = the mean of T over the touched points by a fixed-order reduction; with a NULL target the mean
   sum / touched that ppp_get_path_removal reports for the profile.  From t = 1, `iterations` rounds of a multiplicative update:
     g_i = R_i > 0 ? min(max(T_i / R_i, 2^-6), 2^6) : 1                                   per touched point
     num_j = sum_i llrint((a_ij g_i) 2^28), den_j = sum_i llrint(a_ij 2^28)               signed 64-bit sums over ball j's points
     t_j = min(max(t_j ((double)num_j / (double)den_j), dwell_min), dwell_max)            where den_j > 0; else t_j stays
   with R computed from the rounded products ds_j t_j by the removal's own walk in ascending (slice, sample) order: integer
   sums have no order, so every output is the same bits in every run.  rows[j] (min(row_cap, stats->rows) of them, in (slice,
   sample) order): the slice's index in the walk, the sample's float position, r = the float square root of the r2 its ball
   tests with (NaN: the ball holds nothing, dwell 1), ds, and the final factor.  removal[i] (min(cap, n)): the map the final
   factors predict, 0 for a point no ball holds.  stats: at_min / at_max, min_dwell / max_dwell over the rows with den_j > 0
   (NaN when there are none); residual_before / residual_after = sqrt(mean over the touched points of ((R_i - T_i) / L)^2) at
   t = 1 and at the result (fixed-order sums); path_length = ppp_get_path_removal's; time_factor = (the sum of the rounded
   ds_j t_j, per slice in sample order, the slices in order) / path_length.  touched == 0 or L == 0: every factor stays 1, the
   residuals are NaN, PPP_OK.  The feed cannot raise what lies between two slices: the residual falls to the cross-slice
   ripple of the plan and stays there (7h).  PPP_ERR_ARG: iterations outside [1, 64], bounds that are not finite or not
   0 < dwell_min <= 1 <= dwell_max, an unknown profile, a bad target entry, no pass yet.  PPP_ERR_UNSUPPORTED: a slice-range
   handle (neighbouring ranges share the points of their overlap bands: a range cannot solve alone) and a part handle.
   Otherwise builds, shares and refuses as ppp_get_path_removal does (it asks that call for the unit-feed map first) and
   leaves every other contact result alone.  With a NULL target the result is kept per (pass, profile, iterations, bounds): a
   repeated call launches nothing; with a target every call computes again.  Any output may be NULL. */
typedef struct { int slice; float x, y, z, r; double ds, dwell; } ppp_dwell_row;
typedef struct {
    size_t n, touched, rows;        /* cloud->size(); points a ball holds; rows of the sample table */
    size_t at_min, at_max;          /* rows whose factor ended on a bound */
    int    iterations;
    double level;                   /* L, see above */
    double residual_before, residual_after;   /* sqrt(mean over touched of ((R_i - T_i) / L)^2), at t = 1 and at the result */
    double min_dwell, max_dwell;    /* over rows with den > 0; NaN when there are none */
    double path_length, time_factor;/* sum ds_j ; sum ds_j t_j / sum ds_j, both in (slice, sample) order */
} ppp_dwell_stats;
int ppp_get_path_dwell(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,
                       ppp_dwell_row *rows, size_t row_cap, double *removal, size_t cap, ppp_dwell_stats *stats);
/* A timed feed schedule for the WayPointsList of the last pass: for every row of the list the dwell
   factor there, the feed the tool's contact point may have there under a cap and an acceleration limit, and the time at which
   the waypoint is reached.  Positions are the float rows of PPP_STAGE_WP_XYZ (mm, list order, before hand-eye, smoothing and
   flange offset); the kept slices are the walk's in list order (without the first and the last where drop_ends is set), each
   with the count ppp_get_waypoint_counts gives; a kept slice without waypoints has no rows and is skipped.
     dwell  the rows of ppp_get_path_dwell(profile, target, iterations, dwell_min, dwell_max) on the waypoint's slice, linear in
            (double)y between the last row a with (double)y_a <= y and a + 1 (t_a + u (t_b - t_a), u = (y - y_a) / (y_b - y_a);
            y_b == y_a: t_a); before the first row its factor, at or after the last row its factor; no rows, or a NaN y: 1
     s      (double)S_i 2^-20: S_0 = 0, S_{i+1} = S_i + llrint(d_i 2^20) in signed 64-bit integers along the slice, d_i the double
            distance of waypoints i and i + 1 (differences of the floats in double; 0 when an end is not finite)
     feed   c_i = min(feed / dwell_i, feed_max), at a slice's first and last waypoint also end_feed (>= 0); accel == +INFINITY:
            c_i; else sqrt(min over the slice's j of (c_j c_j + (2 accel) ((double)|S_i - S_j| 2^-20))): the exact
            forward-backward speed limit with braking distance
     limit  what gave the minimum: 0 dwell, 1 feed_max, 2 end (the lowest number on a tie), 3 the acceleration (minimum < c_i c_i)
     t      (the sum of llrint(dt 2^30) over every segment and link before the waypoint in list order) 2^-30.  A segment:
            0 for D_i == 0; 2 sqrt((D_i 2^-20) / accel) when both ends rest; else (2 (D_i 2^-20)) / (v_i + v_{i+1}).  A link,
            from a slice's last waypoint to the first of the next slice that has any: its length l (as d) / link_feed
   Integer sums and minima of exact doubles have no order: every field of every row and of the statistics is the same bits in
   every run.  rows receives the first min(cap, stats->W) rows; cap = 0 with rows == NULL asks for the size (stats->W).  The
   first six arguments are ppp_get_path_dwell's: the call asks that call for its rows, and builds, shares and refuses as it
   does; it leaves every other contact result alone.  PPP_ERR_ARG: no finished ppp_get_path of the handle's last pass, a
   ppp_feed_params field outside its range, fp == NULL.  PPP_ERR_UNSUPPORTED: a slice-range or part handle, and a cloud under
   ppp_trans2center (PPP_STAGE_WP_XYZ is then in the scanner's frame, the dwell rows in the aligned one).  Blocks until the
   results are on the host.  With a NULL target the result is kept per (pass, profile, iterations, bounds, feed parameters): a
   repeated call launches nothing.  Any output may be NULL. */
typedef struct {
    double feed;        /* nominal feed of the contact point, mm/s: finite, > 0 */
    double feed_max;    /* cap on the feed, mm/s: finite, >= feed */
    double accel;       /* limit on |dv/dt| along a slice, mm/s^2: > 0; +INFINITY: no limit */
    double end_feed;    /* cap at the first and last waypoint of every slice, mm/s: finite >= 0; < 0: none */
    double link_feed;   /* feed of the move from a slice's last waypoint to the next slice's first, mm/s: finite, > 0 */
} ppp_feed_params;
typedef struct { int slice; int limit; double dwell, s, feed, t; } ppp_feed_row;   /* one per row of the WayPointsList */
typedef struct {
    size_t W, slices;                 /* waypoints; kept slices with at least one waypoint */
    size_t by_dwell, by_feed_max, by_end, by_accel;   /* waypoints by what binds them (limit 0 / 1 / 2 / 3) */
    double min_feed, max_feed;        /* over all waypoints; NaN when W == 0 */
    double path_length, link_length;  /* mm */
    double duration, duration_links, duration_nominal;  /* s: the whole list; its link moves; path_length / feed */
} ppp_feed_stats;
int ppp_get_path_feed(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,
                      const ppp_feed_params *fp, ppp_feed_row *rows, size_t cap, ppp_feed_stats *stats);
void ppp_default_feed_params(ppp_feed_params *fp);   /* 20, 30, 100, 0, 100 */
/* "x y z r p y t feed " per line: ppp_write_path_file's six columns and format, then t and feed (host only) */
int ppp_write_feed_file(const char *path, const float *wp6, const ppp_feed_row *rows, size_t W);
/* The deviation map of a scan against a reference cloud: for every point of h's resident cloud (the
   scan) its signed distance to the surface of ref's resident cloud (the nominal part, or the scan before the process), that
   distance locally averaged, and a target map that ppp_get_path_dwell and ppp_get_path_feed accept as it is.  p_i is resident
   point i of h, q_j resident point j of ref: the floats each handle holds after its own x1000 and preprocessing.  The two
   clouds are taken as registered in one frame: registration is out of scope.  n_j is row j of ppp_estimate_normals(ref),
   oriented to ref's viewpoint.
     nearest    d2(i, j) = ((dx dx) + dy dy) + dz dz in float; j*(i) is the indexed point of ref with the smallest (d2, j): a tie
                goes to the lower cloud index.  md2 = max_dist * max_dist in float (+INFINITY: no limit).
     status     PPP_DEV_DROPPED if p_i is not finite; PPP_DEV_TOO_FAR if ref indexes no point or d2(i, j*) > md2 (a point at
                exactly md2 matches); PPP_DEV_NO_NORMAL if n_j* has a NaN; otherwise PPP_DEV_MATCHED
     ref_index  j* for MATCHED and NO_NORMAL, -1 otherwise
     deviation  MATCHED points: ((ex nx) + ey ny) + ez nz in double, ex = (double)p.x - (double)q.x and so on: positive where the
                scan lies on the viewpoint's side of the reference surface -- material to take off.  NaN for every other point.
     smoothed   smooth_radius > 0, MATCHED points: N_i = the MATCHED points k of h with d2(p_i, p_k) <= smooth_radius *
                smooth_radius (the float product; i itself belongs to it); ((double)(the sum over N_i of llrint(deviation_k 2^24),
                in signed 64-bit integers) / (double)|N_i|) 2^-24.  NaN for every other point.  smooth_radius == 0: deviation.
     target     gain (v_i - allowance) where that difference is > 0, else +0, v_i = smoothed[i]; +0 for every point that is not
                MATCHED: all entries finite and >= 0
   stats: n = cloud->size() of h; the points by status; proud / below = MATCHED points with v > allowance / v < 0; min_dev /
   max_dev over v (-0 below +0); mean_dev = ((double)(the integer sum of llrint(v_i 2^24)) / (double)matched) 2^-24; rms_dev =
   sqrt(S / matched), S the sum of v_i v_i in the fixed order of ppp_removal_stats' sums; target_sum likewise; max_dist2 = the
   largest float d2 of a MATCHED point; hist[b] = MATCHED points with b = min(63, max(0, (int)floor((v / span + 1) 32))), span =
   max(|min_dev|, |max_dev|), all in bin 32 when span == 0.  NaN for the six numbers when nothing is matched.  Integer sums and
   minima over (d2, j) have no order: every map and every statistic is the same bits in every run.
   Needs clouds and parameters, not a pass.  Builds each handle's slab index, and ref's normal field, where they are missing, as
   ppp_get_contact_field does; a window-path handle stays on the window path.  Waits for ref's stream, runs on h's stream and
   blocks until the results are on the host.  Every call computes again (ref may have changed) and touches no result of the
   other contact calls.  Each map receives its first min(cap, n) entries; every output may be NULL, cap = 0 asks for the
   statistics alone.  h == ref is allowed: every matched deviation is then 0.
   PPP_ERR_ARG: dp or ref NULL; max_dist not > 0 (NaN included); smooth_radius negative or not finite; allowance not finite;
   gain negative or not finite; no cloud on either handle; handles on different devices; smooth_radius > 0 with a max_dist that
   is not finite or with (double)max_dist 2^24 n >= 2^62 (the integer sum could overflow).  PPP_ERR_UNSUPPORTED when either
   handle is a slice-range handle (slice_begin / slice_end; ppp_get_deviation_tile, further down, answers for the points such a
   handle owns) or a part handle (ppp_set_cloud_part). */
enum { PPP_DEV_MATCHED = 0, PPP_DEV_TOO_FAR = 1, PPP_DEV_NO_NORMAL = 2, PPP_DEV_DROPPED = 3 };
typedef struct {
    float  max_dist;       /* mm, resident units: > 0 finite, or +INFINITY for no limit */
    float  smooth_radius;  /* mm: 0 = no smoothing; else > 0 finite */
    double allowance;      /* mm, finite: deviation that is left standing */
    double gain;           /* finite, >= 0: target units per mm of excess */
} ppp_deviation_params;
typedef struct {
    size_t n, matched, too_far, no_normal, dropped;
    size_t proud, below;                 /* matched points with v > allowance ; with v < 0 */
    double min_dev, max_dev;             /* over v of the matched points; NaN when matched == 0 */
    double mean_dev, rms_dev;            /* see above */
    float  max_dist2;                    /* largest float d2 of a matched point; NaN when none */
    double target_sum;
    size_t hist[PPP_CONTACT_BINS];
} ppp_deviation_stats;
void ppp_default_deviation_params(ppp_deviation_params *dp);   /* +INFINITY, 0, 0, 1 */
int  ppp_get_deviation(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp,
                       double *deviation, double *smoothed, int *ref_index, unsigned char *status,
                       double *target, size_t cap, ppp_deviation_stats *stats);
/* The nominal as a resident triangle mesh, and the exact deviation of a scan against it: the closest point on
   the nearest triangle and the distance along that facet's own normal.  No pitch, no estimated normal.
   ppp_trimesh_create: h lends its device, its stream and its change_range; verts / tris are ppp_set_cloud_mesh's (tris NULL = a
   soup, n_verts must be 3 n_tris) and every vertex goes through the same conversion (the x1000 when change_range is set,
   non-finite -> NaN).  After the call the mesh owns its buffers: it depends neither on h nor on any cloud, and nothing that
   replaces, moves or preprocesses a resident cloud touches it.  ppp_trimesh_destroy(NULL) is allowed.
   The triangle frame is 7s's (above): the vertices rotated cyclically so that (p0, p1) is the longest edge, e1 = p1 - p0,
   e2 = p2 - p0, N = e1 x e2, A2 = sqrt((Nx Nx + Ny Ny) + Nz Nz).  Degenerate -- counted, never indexed, never returned -- is
   7s's set: an index outside [0, n_verts), a coordinate that is not finite, A2 zero or not finite.  The facet normal is
   n = (Nx / A2, Ny / A2, Nz / A2); with PPP_TRIMESH_VIEWPOINT it is negated when ((Nx (vx - p0x) + Ny (vy - p0y)) + Nz (vz -
   p0z)) < 0, v = viewpoint in resident units (NULL = the origin); a value of exactly 0 keeps the winding.
   The indexed triangles are listed in a uniform grid of cubic cells of side `cell` over their bounding box, every triangle in
   every cell its axis-aligned box overlaps.  cell = 0 chooses it: the mean longest box side of the indexed triangles, doubled
   until the grid has at most 2^24 cells and fewer than 2^31 - 1 (triangle, cell) pairs.  THE ANSWERS DO NOT DEPEND ON cell:
   the grid decides which triangles a query looks at, not what it finds.  stats: triangles = n_tris = indexed + degenerate;
   cells per axis; pairs and the longest list of one cell; the cell used; the box (resident units).  stats is filled as far as
   the call got.
   PPP_ERR_ARG: out, verts or tp NULL, cell negative or not finite, unknown orient, n_tris == 0, a soup with n_verts != 3 n_tris,
   nothing indexed; PPP_ERR_CAPACITY: more triangles or vertices than (2^31 - 1) / 8, a given cell that breaks either bound
   (never a silent change); PPP_ERR_IO (create_stl = ppp_load_stl + create): a file that cannot be read.  *out is NULL after
   every refusal.

   The search.  All arithmetic is in double, on resident floats widened to double, one rounding per written operation;
   dot(u, v) = (ux vx + uy vy) + uz vz.  For a query p and a triangle in its rotated frame a = p0, b = p1, c = p2 the closest
   point x is Ericson's region walk:
     ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap)
     if d1 <= 0 and d2 <= 0:                       x = a                                   (vertex)
     bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp)
     if d3 >= 0 and d4 <= d3:                      x = b                                   (vertex)
     vc = d1 d4 - d3 d2
     if vc <= 0 and d1 >= 0 and d3 <= 0:           v = d1 / (d1 - d3);  x = a + ab v       (edge)
     cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp)
     if d6 >= 0 and d5 <= d6:                      x = c                                   (vertex)
     vb = d5 d2 - d1 d6
     if vb <= 0 and d2 >= 0 and d6 <= 0:           w = d2 / (d2 - d6);  x = a + ac w       (edge)
     va = d3 d6 - d5 d4
     if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
                                                   w = (d4 - d3) / ((d4 - d3) + (d5 - d6));  x = b + (c - b) w   (edge)
     else:  den = 1 / ((va + vb) + vc);  v = vb den;  w = vc den;  x = (a + ab v) + ac w   (face)
     e = p - x;  D2 = (ex ex + ey ey) + ez ez
   the first test that holds decides.  The winner f* is the indexed triangle with the smallest (D2, f), f its index in the
   caller's list: a tie goes to the lower index.  md2 = (double)max_dist * (double)max_dist (+INFINITY: no limit).
     status     PPP_DEV_DROPPED if the query is not finite; PPP_DEV_TOO_FAR if no indexed triangle has D2 <= md2 (a triangle at
                exactly md2 matches); otherwise PPP_DEV_MATCHED.  PPP_DEV_NO_NORMAL cannot occur.
     matched    tri_index = f*; region = 0 face, 1 edge, 2 vertex; distance = sqrt(D2); closest = x (three doubles);
                deviation = ((ex nx) + ey ny) + ez nz with f*'s facet normal n.  In the face region the deviation is the signed
                distance; on an edge or a vertex it is the component along the winning facet's normal -- 7j's convention, "along
                the normal of the nearest reference element" --, and distance and region say which case applies.  Pseudonormals
                and inside / outside of closed meshes: ppp_trimesh_signed_nearest, below.
     otherwise  tri_index -1, region 255, every double the one quiet NaN of the deviation maps.
   Minima over (D2, f) have no order: the maps are the same bits in every run and for every cell.
   ppp_trimesh_nearest: the primitive.  n packed xyz points in RESIDENT units (no x1000) against the mesh, on the mesh's own
   stream; every output may be NULL; blocks.  PPP_ERR_ARG: m NULL, xyz NULL with n > 0, max_dist not > 0.
   ppp_get_mesh_deviation: the search over h's resident cloud (its points in the handle's slab order), then ppp_get_deviation's
   own tail: smoothed, target and every field of stats->dev are defined by that call's comment word for word, with MATCHED
   read as "matched to a triangle", no_normal = 0 and max_dist2 = (float)D2 of the farthest matched point.  on_face + on_edge
   + on_vertex = matched; max_distance = the largest distance (NaN when nothing matched).  Each map receives its first
   min(cap, n) entries; every output may be NULL, cap = 0 asks for the statistics alone.  Needs a cloud and parameters, not a
   pass; builds h's slab index where it is missing; runs on h's stream, blocks, keeps nothing.
   PPP_ERR_ARG: m or dp NULL, ppp_get_deviation's conditions on dp (the integer-sum guard included), no cloud, a mesh on another
   device than h.  PPP_ERR_UNSUPPORTED: a slice-range or a part handle. */
typedef struct ppp_trimesh_s *ppp_trimesh;
enum { PPP_TRIMESH_WINDING = 0, PPP_TRIMESH_VIEWPOINT = 1 };
typedef struct { float cell; int orient; } ppp_trimesh_params;          /* defaults 0 (= automatic), PPP_TRIMESH_WINDING */
typedef struct { size_t triangles, indexed, degenerate; size_t cells[3]; size_t pairs, max_per_cell;
                 float cell; float mn[3], mx[3]; } ppp_trimesh_stats;
void ppp_default_trimesh_params(ppp_trimesh_params *tp);
int  ppp_trimesh_create(ppp_handle h, const float *verts, size_t n_verts, const int *tris, size_t n_tris,
                        const ppp_trimesh_params *tp, const float *viewpoint, ppp_trimesh *out, ppp_trimesh_stats *stats);
int  ppp_trimesh_create_stl(ppp_handle h, const char *path, const ppp_trimesh_params *tp, const float *viewpoint,
                            ppp_trimesh *out, ppp_trimesh_stats *stats);
void ppp_trimesh_destroy(ppp_trimesh m);
int  ppp_trimesh_nearest(ppp_trimesh m, const float *xyz, size_t n, float max_dist,
                         double *distance, double *closest, double *deviation, int *tri_index,
                         unsigned char *region, unsigned char *status);
typedef struct { ppp_deviation_stats dev; size_t on_face, on_edge, on_vertex; double max_distance; } ppp_mesh_deviation_stats;
int  ppp_get_mesh_deviation(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp,
                            double *deviation, double *smoothed, double *distance, int *tri_index,
                            unsigned char *region, unsigned char *status, double *target, size_t cap,
                            ppp_mesh_deviation_stats *stats);
/* Signed distance to a triangle mesh: welded topology, angle-weighted pseudonormals (Baerentzen and Aanaes), and the sign they
   give the exact search's distance.  ppp_trimesh_nearest and ppp_get_mesh_deviation are untouched; these are
   calls beside them.
   The topology is built once per mesh, on the mesh's stream, in the mesh's own buffers (freed by ppp_trimesh_destroy):
   explicitly by ppp_trimesh_topology, or by the first of the other three calls that needs it.  Only indexed triangles take
   part.  All arithmetic is in double on resident floats widened to double, one rounding per written operation;
   dot(u, v) = (ux vx + uy vy) + uz vz, cross(u, v) = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), |u| = sqrt(dot(u, u)).
     corner     corner k (0, 1, 2: the caller's corner order) of triangle f (the caller's list) has the corner index 3 f + k.
     weld       two corners are one vertex when their resident floats compare equal on all three axes (-0 equals +0; no
                tolerance).  The vertex id is the smallest corner index at that position.
     half-edge  half-edge k of f runs from corner k to corner (k + 1) % 3; where PPP_TRIMESH_VIEWPOINT negated f's normal it
                runs the other way.  An edge is the unordered pair of vertex ids; its id is the smallest 3 f + k among its
                half-edges.
     class      PPP_EDGE_BORDER: one half-edge; PPP_EDGE_MANIFOLD: two that run in opposite directions;
                PPP_EDGE_INCONSISTENT: two that run the same way; PPP_EDGE_NONMANIFOLD: more than two.
     vertex bits  PPP_VERTEX_BORDER: on a border edge; PPP_VERTEX_IRREGULAR: on an inconsistent or a non-manifold edge.
     n_f        f's facet normal exactly as the search forms it (N / A2 of the rotated frame, negated by the orient rule).
     edge pseudonormal    s = (0, 0, 0); for its half-edges in ascending 3 f + k: s = s + n_f, per component.
     vertex pseudonormal  s = (0, 0, 0); for its corners in ascending 3 f + k: s = s + alpha n_f, per component, with
                alpha = atan2(|cross(u, v)|, dot(u, v)), u = corner (k + 1) % 3 - corner k, v = corner (k + 2) % 3 - corner k.
                Both are left unnormalised: only the sign of a product with them is used.
   Every sum has a fixed order: the values are the same bits in every run and for every cell.
   ppp_trimesh_topology_stats: the counts of vertices, edges, edges by class, border and irregular vertices; closed = 1 when
   there is no border, inconsistent or non-manifold edge -- ONLY THEN does the sign below mean inside (negative) / outside of
   a solid whose facets are wound counter-clockwise seen from outside.
   ppp_trimesh_get_topology: per triangle and corner of the caller's list, the first min(cap, n_tris) triangles, [cap][3] each:
   vertex_id and edge_id (of half-edge k) as corner indices, edge_class, vertex_bits, and [cap][3][3] the vertex's and the edge's
   pseudonormal.  A degenerate triangle's rows are -1, 255 and NaN.  Every output may be NULL; stats too.
   PPP_ERR_ARG (both): m NULL.

   The signed query.  Behind the search (k_mesh_nearest, unchanged) one more launch, a thread per query: for a MATCHED query it
   walks the winner f* again (the same inputs and arithmetic: the same x, D2 and region) and notes the feature x lies on;
     g          face: n_f*; edge: that edge's pseudonormal; vertex: that vertex's pseudonormal;
     s          dot(e, g), e = p - x;
     signed_distance  copysign(distance, s) when s > 0 or s < 0 and g is not the zero vector; otherwise copysign(distance,
                deviation) -- the search's deviation, a +0 counts as positive -- and PPP_MESH_SIGN_FALLBACK is set (a query on
                the mesh itself, an edge whose facets cancel);
     feature    0 .. 2: the caller's corner x is; 3 + k: x lies on the caller's half-edge k; 6: in the face;
     flags      PPP_MESH_SIGN_BORDER: x is on a border edge or a border vertex; PPP_MESH_SIGN_IRREGULAR: on an inconsistent or
                non-manifold edge, or an irregular vertex; PPP_MESH_SIGN_FALLBACK: as above;
     pseudonormal  g, three doubles.
   A query that is not matched gets NaN, feature 255, flags 0.
   ppp_trimesh_signed_nearest: ppp_trimesh_nearest with the four maps in front; its own six outputs are that call's bits.  Every
   output may be NULL.  PPP_ERR_ARG: m NULL, xyz NULL with n > 0, max_dist not > 0.
   ppp_get_mesh_signed_deviation: ppp_get_mesh_deviation word for word with signed_distance in the place of deviation: the sign
   launch rewrites the deviation map and its fixed-point term before the tail runs, so smoothed, target and every field of
   stats->mesh.dev are computed from the signed distance; distance, tri_index, region, status, on_face / on_edge / on_vertex
   and max_distance are ppp_get_mesh_deviation's.  feature and flags as above (255 and 0 where not matched).  Of the matched
   points: on_border, irregular and fallback count the flags, negative those with signed_distance < 0, positive those > 0.
   Cap semantics and refusals are ppp_get_mesh_deviation's: PPP_ERR_ARG: m or dp NULL, ppp_get_deviation's conditions on dp, no
   cloud, a mesh on another device than h; PPP_ERR_UNSUPPORTED: a slice-range or a part handle. */
enum { PPP_EDGE_BORDER = 0, PPP_EDGE_MANIFOLD = 1, PPP_EDGE_INCONSISTENT = 2, PPP_EDGE_NONMANIFOLD = 3 };
enum { PPP_VERTEX_BORDER = 1, PPP_VERTEX_IRREGULAR = 2 };
enum { PPP_MESH_SIGN_BORDER = 1, PPP_MESH_SIGN_IRREGULAR = 2, PPP_MESH_SIGN_FALLBACK = 4 };
typedef struct { size_t vertices, edges, border_edges, manifold_edges, inconsistent_edges, nonmanifold_edges,
                 border_vertices, irregular_vertices; int closed; } ppp_trimesh_topology_stats;
int  ppp_trimesh_topology(ppp_trimesh m, ppp_trimesh_topology_stats *stats);
int  ppp_trimesh_get_topology(ppp_trimesh m, int *vertex_id, int *edge_id, unsigned char *edge_class,
                              unsigned char *vertex_bits, double *vertex_normal, double *edge_normal, size_t cap,
                              ppp_trimesh_topology_stats *stats);
int  ppp_trimesh_signed_nearest(ppp_trimesh m, const float *xyz, size_t n, float max_dist,
                                double *signed_distance, double *pseudonormal, unsigned char *feature, unsigned char *flags,
                                double *distance, double *closest, double *deviation, int *tri_index,
                                unsigned char *region, unsigned char *status);
typedef struct { ppp_mesh_deviation_stats mesh; size_t on_border, irregular, fallback, negative, positive; } ppp_mesh_signed_deviation_stats;
int  ppp_get_mesh_signed_deviation(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp,
                                   double *signed_distance, double *smoothed, double *distance, int *tri_index,
                                   unsigned char *region, unsigned char *feature, unsigned char *flags,
                                   unsigned char *status, double *target, size_t cap,
                                   ppp_mesh_signed_deviation_stats *stats);
/* Registration of a scan to a reference cloud: point-to-plane ICP.  h holds the scan, ref the nominal
   cloud (or the scan before the process); the result T = (R | t), row-major 3 x 4 in double, carries a resident point of h into
   ref's frame.  ppp_get_deviation does not register; these calls do, and ppp_transform_cloud applies their result.  ICP is a
   local method: it needs a start T0 within the basin of the answer -- a fixturing error of millimetres and a few degrees, not
   an unknown pose; ppp_register_global, further down, finds one.  Everything below is + - * / in double with one rounding per
   written operation, and integers wherever a sum has no fixed order: the same bits in every run.
     centre     mn, mx = ppp_minmax(ref); c[d] = ((double)mn[d] + (double)mx[d]) * 0.5; e = (double)mx - (double)mn;
                Ln = (((ex + ey) + ez) * 0.5) + (double)max_dist
     shift      min(40, 60 - clog2(max(2, n)) - clog2(max(1, ceil((double)(max_dist * max_dist))))), the product in float, n =
                cloud->size() of h, clog2(x) the smallest e with 2^e >= x; the fixed point is 2^shift
     moved      p an indexed (finite) point of h: p'[r] = ((T[4r] px + T[4r+1] py) + T[4r+2] pz) + T[4r+3]; the query is (float)p';
                a query that is not finite is no pair
     pair       j* = the nearest indexed point of ref to the query under ppp_get_deviation's rule (float d2, a point at exactly
                max_dist * max_dist matches, a tie goes to the lower index); a pair where j* exists and row j* of
                ppp_estimate_normals(ref), n, has no NaN
     terms      e = p' - (double)q; r = ((ex nx) + ey ny) + ez nz; u[d] = (p'[d] - c[d]) / Ln; a = (uy nz - uz ny, uz nx - ux nz,
                ux ny - uy nx); J = (a, n); A_ik += llrint((J_i J_k) 2^shift), b_i += llrint((J_i r) 2^shift),
                E += llrint((r r) 2^shift), pairs += 1
     solve      M = (double)A, g = -(double)b, big = the largest M_ii; LDL^T in index order: v = M_ii - (the sum over the
                unlocked k < i, ascending, from 0, of (L_ik L_ik) d_k); !(v > lock_eps big) locks i: x_i = 0 and i takes no part
                in any later sum; else d_i = v, L_ji = (M_ji - the sum over the unlocked k < i of (L_jk L_ik) d_k) / v;
                z_i = g_i - the sum of L_ik z_k; x_i = z_i / d_i - the sum over the unlocked k > i, ascending, of L_ki x_k
     no step    from an evaluation with pairs < 6 or all six unknowns locked (the loop ends, converged = 0), and from one whose
                six b are all zero with pairs >= 6 (T is a stationary point: the loop ends, converged = 1)
     step       w = x[0..2] / Ln, h = w * 0.5, s = (hx hx + hy hy) + hz hz, dR = ((1 - s) I + 2 h h^T + 2 [h]x) / (1 + s) (Cayley's
                form, every entry (diagonal + 2 (h_i h_j) +- 2 h_k) / (1 + s)), dt = x[3..5]; R' = dR R, each entry
                ((a0 b0) + a1 b1) + a2 b2; t' = (dR (t - c) + c) + dt; step2 = max((x0 x0 + x1 x1) + x2 x2, (x3 x3 + x4 x4) + x5 x5);
                the loop ends after a step with step2 < min_step * min_step (converged = 1), else after `iterations` steps
   ppp_get_registration_terms evaluates once at T12 (NULL: the identity) and takes no step: *row is that evaluation (locked 63,
   step2 NaN); stats has n, indexed, shift, centre, length, T = T12, steps = converged = locked = 0 and the row's numbers in both
   the _before and the _after fields.  ppp_register runs the loop from T0_12 (NULL: the identity): rows[k] holds the terms at T_k
   for k = 0 .. steps, the last of them the evaluation at the result (locked 63, step2 NaN); the first min(row_cap, steps + 1)
   rows are copied, rows may be NULL with row_cap = 0; stats.locked is the OR of the masks of the rows a step was taken from.
   Both build each handle's slab index and ref's normal field where they are missing, wait once for ref's stream, enqueue the
   whole chain (iterations + 1 evaluations, iterations steps, no host round trip per iteration) on h's stream and wait once.
   Neither changes either handle's cloud, plan or any stored contact result.  h == ref is allowed: row 0 has b = 0 and E = 0.
   row, rows and stats may be NULL.  PPP_ERR_ARG: rp or ref NULL; rows NULL with row_cap > 0; max_dist not finite and > 0, or its float
   square not finite; iterations outside [1, 64]; min_step not finite and >= 0; lock_eps outside (0, 1); a T entry that is not
   finite; no cloud on either handle; handles on different devices; shift < 16 (the integer sums could overflow).
   PPP_ERR_UNSUPPORTED when either handle is a slice-range handle or a part handle. */
typedef struct {
    float  max_dist;     /* mm, resident units: finite, > 0: a scan point pairs with a reference point within it */
    int    iterations;   /* at most this many steps: 1 .. 64 */
    double min_step;     /* mm, finite, >= 0: stop once a step moves nothing farther than this */
    double lock_eps;     /* in (0, 1): pivot rule of the solve, see below */
} ppp_registration_params;                       /* defaults: 2, 30, 1e-6, 1e-9 */

typedef struct {
    double    T[12];     /* row-major 3 x 4 (R | t): the transform the terms were taken at */
    size_t    pairs;
    long long A[21];     /* upper triangle of J^T J, row-major (00 01 .. 05 11 12 .. 55), fixed point */
    long long b[6];      /* J^T r */
    long long E;         /* r^T r */
    int       locked;    /* bit i: unknown i took no step here (pivot rule); 63 on a row no step was taken from */
    double    step2;     /* max(|scaled rotation|^2, |translation|^2) of the step taken from here; NaN: none */
} ppp_registration_row;

typedef struct {
    size_t n, indexed;                  /* scan: cloud->size(), finite points */
    int    steps, converged, locked;    /* steps taken; step2 < min_step^2 reached; OR of the rows' masks */
    int    shift;                       /* the fixed point is 2^shift */
    double centre[3], length;           /* c and Ln below */
    double T[12];                       /* the result: scan -> reference frame */
    size_t pairs_before, pairs_after;
    double rms_before, rms_after;       /* sqrt((double)E 2^-shift / pairs) at T0 and at T; NaN when pairs == 0 */
} ppp_registration_stats;

void ppp_default_registration_params(ppp_registration_params *rp);
int  ppp_get_registration_terms(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T12,
                                ppp_registration_row *row, ppp_registration_stats *stats);
int  ppp_register(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T0_12,
                  ppp_registration_row *rows, size_t row_cap, ppp_registration_stats *stats);
/* Registration of a scan to the triangle mesh itself: point-to-plane ICP on the facets that
   ppp_get_mesh_deviation measures against.  h holds the scan, m is a ppp_trimesh; no pitch, no sampled cloud and no estimated
   normal enter the fit.  Everything is ppp_register's, word for word, except:
     centre     mn, mx = the mesh's box (m's ppp_trimesh_stats mn / mx, floats widened): c[d] = (mn[d] + mx[d]) * 0.5;
                Ln = (((ex + ey) + ez) * 0.5) + (double)max_dist, e = mx - mn
     shift      ppp_register's (n = cloud->size() of h, the product max_dist * max_dist in float); shift < 16 is refused
     moved      p'[r] = ((T[4r] px + T[4r+1] py) + T[4r+2] pz) + T[4r+3] in double, and THE QUERY IS p' ITSELF, in double, not its
                float (at T = identity p' is the point's float widened, exactly); a p' that is not finite is no pair
     pair       f* = the nearest indexed triangle of m to p' by (D2, f) -- the search of ppp_get_mesh_deviation's comment, the
                brute force's answer over all indexed triangles whatever the cell -- with x its closest point; a pair where
                D2 <= (double)max_dist * (double)max_dist (inclusive).  Every region pairs: face, edge and vertex
     terms      q = x (double); n = (Nx / A2, Ny / A2, Nz / A2) of f*'s frame; e = p' - x; r = ((ex nx) + ey ny) + ez nz; u, a, J and
                the 21 + 6 + 1 words with llrint(... 2^shift) are ppp_register's expressions on these doubles
     orientation  PPP_TRIMESH_WINDING or _VIEWPOINT is NOT applied, and need not be: n -> -n negates J and r together, a
                negation is exact, so every product J_i J_k, J_i r and r r is the same double either way, and so is every word:
                a mesh made with either orientation gives the same rows
   Solve, step, composition, the loop's endings, rows and stats are ppp_register's.  On an edge or a vertex the normal is the
   winning facet's (pseudonormals are out of scope), and the scan's overhang beyond an open mesh's border pairs there with the
   border facet's normal as long as it lies within max_dist (no pair is rejected on the border here).  Robust weights are
   ppp_register_mesh_robust's, trimmed weights and the rejection of border pairs ppp_register_mesh_trimmed's (both below), the
   start from an unknown pose is ppp_register_mesh_global's (further down); tiles over slice ranges are ppp_register_mesh_tiles's
   (further down).
   ppp_get_mesh_registration_terms evaluates once at T12 (NULL: the identity) and takes no step; ppp_register_mesh runs the loop
   from T0_12; row, rows and stats are filled as ppp_get_registration_terms and ppp_register fill them.  Both build h's slab index
   where it is missing, enqueue the whole chain (iterations + 1 evaluations, iterations steps) on h's stream and wait once; the
   mesh is read-only after its create call.  Neither changes h's cloud, plan or stored results, nor the mesh.
   PPP_ERR_ARG: m or rp NULL; rows NULL with row_cap > 0; ppp_register's parameter ranges; a T entry that is not finite; no cloud
   on h; a mesh on another device than h; shift < 16.  PPP_ERR_UNSUPPORTED: a slice-range or a part handle. */
int  ppp_get_mesh_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T12,
                                     ppp_registration_row *row, ppp_registration_stats *stats);
int  ppp_register_mesh(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T0_12,
                       ppp_registration_row *rows, size_t row_cap, ppp_registration_stats *stats);
/* Trimmed registration: ppp_register's loop in which only the share `keep` of an evaluation's pairs
   with the smallest pair distance enters its sums (trimmed ICP, Chetverikov et al.).  A scan from a cell carries what the
   reference does not show -- a clamp pad, a strip of the table, a burr, an edge -- within max_dist of it; such points pair, pull
   ppp_register's fit, and are cut off here as long as keep lies below the share of the scan that does show the reference.
     pair       ppp_register's, word for word (moved, the float query, the nearest point and its tie rule, a point at exactly
                max_dist * max_dist matches, no pair where the normal has a NaN or the query is not finite); paired = their number
     key        the bit pattern of the pair's float d2 as a 32-bit unsigned integer: d2 is a sum of squares, never negative and
                never NaN, so the keys order as the floats do
     cut        k = (size_t)ceil(keep * (double)paired), one double product and one ceil, clamped to [1, paired]; tau = the k-th
                smallest key (1-based); KEPT = the pairs with key <= tau: every pair that ties with the k-th is kept, kept >= k,
                and nothing depends on an order among equal keys; trim_d2 = the float with the bits of tau.  paired == 0:
                kept = 0 and trim_d2 is the float quiet NaN 0x7fc00000 (the double 0x7ff8000000000000 of step2, narrowed)
     terms      ppp_register's 29 words over the KEPT pairs only, row.pairs = kept; shift, centre and Ln are ppp_register's for
                the same n and max_dist
     the rest   solve, step, composition and the loop's endings are ppp_register's with pairs read as kept ("fewer than 6
                pairs" is kept < 6); stats is ppp_register's with pairs_* = kept and rms_* over the kept pairs
     maps       status and d2, by cloud index of h, the first min(cap, n) entries, of the LAST evaluation (the one at the
                result, rows[steps]): PPP_TRIM_DROPPED and NaN for a point that is not finite, PPP_TRIM_UNPAIRED and NaN for
                one without a pair, else PPP_TRIM_KEPT or PPP_TRIM_TRIMMED and the pair's float d2 (every NaN is 0x7fc00000).
                A caller masks ppp_get_deviation's maps with them.
   keep == 1 keeps every pair: rows[k].row, T and stats are ppp_register's bits from the same start.  rows, status, d2 and stats
   may be NULL (rows with row_cap = 0; status and d2 with any cap).  The whole chain -- per evaluation the search with the top
   digit's histogram, two passes over the stored keys, the sums, the step -- is enqueued at once on h's stream with one wait at
   its end; neither handle's cloud, plan or stored results change.  PPP_ERR_ARG: ppp_register's refusals; tp NULL; keep NaN,
   <= 0 or > 1.  PPP_ERR_UNSUPPORTED when either handle is a slice-range handle or a part handle. */
typedef struct {
    ppp_registration_params icp;   /* ppp_register's four, with its ranges */
    double keep;                   /* in (0, 1]: the share of an evaluation's pairs that enter its sums */
} ppp_trimmed_registration_params;          /* defaults: ppp_default_registration_params, 0.8 */

typedef struct {
    ppp_registration_row row;      /* as ppp_register's, but pairs / A / b / E are over the KEPT pairs */
    size_t paired;                 /* pairs found by the search at row.T (what ppp_register would sum) */
    float  trim_d2;                /* the cut: the largest float d2 that is kept; NaN when paired == 0 */
} ppp_trimmed_registration_row;

enum { PPP_TRIM_KEPT = 0, PPP_TRIM_TRIMMED = 1, PPP_TRIM_UNPAIRED = 2, PPP_TRIM_DROPPED = 3 };

void ppp_default_trimmed_registration_params(ppp_trimmed_registration_params *tp);
int  ppp_register_trimmed(ppp_handle h, ppp_handle ref, const ppp_trimmed_registration_params *tp, const double *T0_12,
                          ppp_trimmed_registration_row *rows, size_t row_cap,
                          unsigned char *status, float *d2, size_t cap,
                          ppp_registration_stats *stats);
/* Robust registration: ppp_register's loop in which every pair enters the sums with Tukey's
   biweight of its point-to-plane residual, the scale being the median absolute residual of each evaluation.  Nothing has to
   choose a share of the scan beforehand, as ppp_register_trimmed's keep does: what the reference does not show -- a clamp pad, a
   strip of the table, a burr -- ends at weight 0 once the fit has tightened around the rest.  The estimator's limit: it needs
   the median residual to belong to the part that shows the reference.  With a third of the scan raised by 1.5 mm the median
   residual is about 0.5 mm, the fit tilts and stays tilted; ppp_register_trimmed with a known keep remains the
   tool for heavy contamination.
     pair       ppp_register's, word for word (moved, the float query, the nearest point and its tie rule, a point at exactly
                max_dist * max_dist matches, no pair where the normal has a NaN or the query is not finite); paired = their number
     residual   r = ((ex nx) + ey ny) + ez nz, ppp_register's double
     key        the bit pattern of (float)fabs(r) as a 32-bit unsigned integer: never negative and never NaN, so the keys order
                as the floats do
     scale      k = ppp_trim_rank(0.5, paired); tau = the k-th smallest key (1-based), found through ppp_register_trimmed's three
                digit histograms; m = (double) the float with the bits of tau (median_abs); sigma = max(1.4826 * m, sigma_min);
                cs = tune * sigma.  paired == 0: median_abs is the float quiet NaN 0x7fc00000, sigma the double quiet NaN
                0x7ff8000000000000, and no step is taken
     weight     tune == +INFINITY: w = 1.  cs == 0: w = 1 where r == 0, else 0.  Otherwise u = r / cs, v = 1 - u * u,
                w = fabs(u) < 1 ? v * v : 0; one rounding per written operation, no transcendental
     terms      A_ik += llrint(((J_i J_k) w) 2^shift), b_i += llrint(((J_i r) w) 2^shift), E += llrint(((r r) w) 2^shift),
                weight_sum += llrint(w 2^shift); row.pairs = paired; used = the pairs with w > 0; shift, centre, Ln and J are
                ppp_register's.  With w = 1 every product is exact in that order: the words are ppp_register's
     the rest   solve, step, composition and the loop's endings are ppp_register's with "fewer than 6 pairs" read as used < 6;
                stats is ppp_register's with pairs_* = paired and rms_* = sqrt((double)E / (double)weight_sum), NaN when
                weight_sum == 0
     maps       status, weight and residual, by cloud index of h, the first min(cap, n) entries, of the LAST evaluation (the one
                at the result, rows[steps]): PPP_ROBUST_DROPPED for a point that is not finite, PPP_ROBUST_UNPAIRED for one
                without a pair, else PPP_ROBUST_USED (w > 0) or PPP_ROBUST_REJECTED (w == 0); weight is (float)w and residual
                is r, the float NaN 0x7fc00000 and the double NaN 0x7ff8000000000000 where there is no pair
   tune == +INFINITY weighs every pair 1: rows[k].row, T and stats are ppp_register's bits from the same start.
   ppp_get_robust_registration_terms evaluates once at T12 (NULL: the identity) and takes no step, as
   ppp_get_registration_terms does; its maps are that evaluation's.  rows, row, the maps and stats may be NULL (rows with
   row_cap = 0; the maps with any cap).  The whole chain -- per evaluation the search with the top digit's histogram, two passes
   over the stored keys, the weighted sums, the step -- is enqueued at once on h's stream with one wait at its end; neither
   handle's cloud, plan or stored results change.  PPP_ERR_ARG: ppp_register's refusals; bp NULL; tune NaN or <= 0 (+INFINITY
   is allowed); sigma_min not finite or < 0.  PPP_ERR_UNSUPPORTED when either handle is a slice-range handle or a part handle. */
typedef struct {
    ppp_registration_params icp;   /* ppp_register's four, with its ranges */
    double tune;                   /* > 0, +INFINITY allowed: the cut of the biweight in units of sigma */
    double sigma_min;              /* mm, finite, >= 0: the floor of sigma */
} ppp_robust_registration_params;           /* defaults: ppp_default_registration_params, 4.685, 1e-4 */

typedef struct {
    ppp_registration_row row;      /* as ppp_register's: pairs = paired, A / b / E weighted */
    size_t    used;                /* pairs with a weight above zero */
    long long weight_sum;          /* the sum of the weights, fixed point */
    float     median_abs;          /* the median of |r| as a float; NaN when paired == 0 */
    double    sigma;               /* max(1.4826 * median_abs, sigma_min); NaN when paired == 0 */
} ppp_robust_registration_row;

enum { PPP_ROBUST_USED = 0, PPP_ROBUST_REJECTED = 1, PPP_ROBUST_UNPAIRED = 2, PPP_ROBUST_DROPPED = 3 };

void ppp_default_robust_registration_params(ppp_robust_registration_params *bp);
int  ppp_get_robust_registration_terms(ppp_handle h, ppp_handle ref, const ppp_robust_registration_params *bp, const double *T12,
                                       ppp_robust_registration_row *row,
                                       unsigned char *status, float *weight, double *residual, size_t cap,
                                       ppp_registration_stats *stats);
int  ppp_register_robust(ppp_handle h, ppp_handle ref, const ppp_robust_registration_params *bp, const double *T0_12,
                         ppp_robust_registration_row *rows, size_t row_cap,
                         unsigned char *status, float *weight, double *residual, size_t cap,
                         ppp_registration_stats *stats);
/* Robust registration of a scan to the triangle mesh itself: ppp_register_mesh's pairs on the
   facets under ppp_register_robust's weights, for a scan that shows what the mesh does not -- a clamp pad, a strip of the
   table, a burr -- within max_dist of it.  No struct or enum is new: the parameters, the row and PPP_ROBUST_* are
   ppp_register_robust's.
     centre, shift, moved, pair   ppp_register_mesh's, word for word: the frame from the mesh's box; ppp_register's shift,
                shift < 16 refused; the query is the moved point p' itself, in double; the winner is the nearest indexed
                triangle by (D2, f) with its exact closest point x; a pair where D2 <= (double)max_dist * (double)max_dist
                (inclusive), in every region; paired = their number
     residual   r = ((ex nx) + ey ny) + ez nz with e = p' - x and n = N / A2 of the winning record's own frame:
                ppp_register_mesh's double
     key, scale, weight, terms    ppp_register_robust's, word for word: the key is the bits of (float)fabs(r); k =
                ppp_trim_rank(0.5, paired) through the three digit histograms; sigma = max(1.4826 * m, sigma_min), cs = tune *
                sigma; w as there; 30 words, each product times w before llrint(... 2^shift), with ppp_register_mesh's u and J on
                doubles; used = the pairs with w > 0, which is what the step reads as its pairs.  paired == 0: median_abs is the
                float quiet NaN 0x7fc00000, sigma the double quiet NaN 0x7ff8000000000000, and no step is taken
     rows, stats, maps, endings   ppp_register_robust's: row.pairs = paired; rms_* = sqrt((double)E / (double)weight_sum); the maps
                by cloud index of h from the LAST evaluation; PPP_ROBUST_DROPPED for a point that is not finite,
                PPP_ROBUST_UNPAIRED for one without a pair and for one whose moved point is not finite
     orientation  PPP_TRIMESH_WINDING or _VIEWPOINT is NOT applied.  Flipping a facet negates r and J together: |r|, the key, w
                (even in r) and every product are unchanged, so every word and every row is the same either way.  The residual
                MAP is signed by the record's own normal (its winding as given), so it is negated where the facet is flipped
   tune == +INFINITY weighs every pair 1: rows[k].row, T and stats are ppp_register_mesh's bits from the same start.  Every
   output is the same for every grid cell of the mesh, and the same bits in every run.  The estimator's limit is
   ppp_register_robust's: the median residual must belong to the part that shows the mesh (with 35 % of the scan raised by 1.5 mm
   it does not, and the fit stays tilted): there ppp_register_mesh_trimmed (below) with a known keep is the
   tool, and it rejects border pairs too.  Tiles over slice ranges and pseudonormals are not offered; the start from an unknown
   pose is ppp_register_mesh_global's (further down).
   ppp_get_mesh_robust_registration_terms evaluates once at T12 (NULL: the identity) and takes no step; its maps are that
   evaluation's.  rows, row, the maps and stats may be NULL (rows with row_cap = 0; the maps with any cap).  The whole chain -- per
   evaluation the grid walk, paid once, with the residual, the key and the top digit's histogram, two passes over the stored
   keys, the weighted sums over the stored winners, the step -- is enqueued at once on h's stream with one wait at its end.
   Neither call changes h's cloud, plan or stored results, nor the mesh.
   PPP_ERR_ARG: m or bp NULL; rows NULL with row_cap > 0; ppp_register's parameter ranges; tune NaN or <= 0 (+INFINITY is
   allowed); sigma_min not finite or < 0; a T entry that is not finite; no cloud on h; a mesh on another device than h;
   shift < 16.  PPP_ERR_UNSUPPORTED: a slice-range or a part handle. */
int  ppp_get_mesh_robust_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T12,
                                            ppp_robust_registration_row *row,
                                            unsigned char *status, float *weight, double *residual, size_t cap,
                                            ppp_registration_stats *stats);
int  ppp_register_mesh_robust(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T0_12,
                              ppp_robust_registration_row *rows, size_t row_cap,
                              unsigned char *status, float *weight, double *residual, size_t cap,
                              ppp_registration_stats *stats);
/* Trimmed registration of a scan to the triangle mesh itself, with border-pair rejection:
   ppp_register_mesh's candidates on the facets under ppp_register_trimmed's cut, for a scan that is heavily contaminated -- more
   than the median of ppp_register_mesh_robust bears -- and whose share `keep` that shows the mesh is known; and, with
   border = PPP_MESH_BORDER_REJECT, for a scan that shows more than an open mesh does: a candidate whose closest point lies on
   the mesh's border is no pair (Turk and Levoy), whatever its point-to-plane residual against the border facet's extrapolated
   plane would be.
     centre, shift, moved, candidate   ppp_register_mesh's, word for word: the frame from the mesh's box; ppp_register's shift,
                shift < 16 refused; the query is the moved point p' itself, in double; the winner f* is the nearest indexed
                triangle by (D2, f) with its exact closest point x; a candidate where D2 <= (double)max_dist * (double)max_dist
                (inclusive), in every region
     border     PPP_MESH_BORDER_PAIR: every candidate is a pair, as in ppp_register_mesh; no topology is built and on_border is 0.
                PPP_MESH_BORDER_REJECT: the mesh's welded topology is built where it is missing, as
                ppp_get_mesh_signed_deviation builds it; the winner's record is walked once more for the feature x lies on --
                the same inputs and the same arithmetic, so x, D2 and the region are the walk's bits --; a candidate is NO pair
                where that feature is a vertex with PPP_VERTEX_BORDER or an edge of class PPP_EDGE_BORDER: exactly where
                ppp_get_mesh_signed_deviation sets PPP_MESH_SIGN_BORDER.  Its status is PPP_MESH_TRIM_BORDER, its d2 the float
                NaN 0x7fc00000, it is counted in on_border and is not part of paired.  Inconsistent and non-manifold features
                are not rejected.  On a mesh whose topology has no border edge _REJECT gives _PAIR's bits
     key        the bit pattern of (float)D2, the walk's double narrowed once, as a 32-bit unsigned integer: never negative and
                never NaN, and round-to-nearest is monotone, so the keys order as the distances do; ties are kept together
     cut        ppp_register_trimmed's: k = ppp_trim_rank(keep, paired), tau = the k-th smallest key through the three digit
                histograms, KEPT = the pairs with key <= tau, kept >= k; trim_d2 = the float with the bits of tau, the float
                quiet NaN 0x7fc00000 when paired == 0
     terms      ppp_register_mesh's 29 words -- q = x, n = N / A2 of f*'s frame, u and J on doubles -- over the KEPT pairs only,
                row.pairs = kept
     the rest   solve, step, composition and the loop's endings are ppp_register's with pairs read as kept ("fewer than 6
                pairs" is kept < 6); stats is ppp_register's with pairs_* = kept and rms_* over the kept pairs
     maps       status and d2, by cloud index of h, the first min(cap, n) entries, of the LAST evaluation (the one at the
                result, rows[steps]): PPP_TRIM_DROPPED and NaN for a point that is not finite, PPP_TRIM_UNPAIRED and NaN for one
                without a candidate (a moved point that is not finite too), PPP_MESH_TRIM_BORDER and NaN for a candidate
                rejected on the border, else PPP_TRIM_KEPT or PPP_TRIM_TRIMMED and the key's float (every NaN is 0x7fc00000)
     orientation  PPP_TRIMESH_WINDING or _VIEWPOINT is NOT applied, and need not be, for ppp_register_mesh's reason; the class
                of an edge with one half-edge does not depend on a direction, so the BORDER set is the same either way
   With keep == 1 and _PAIR, rows[k].trim.row, T and stats are ppp_register_mesh's bits from the same start.  Every output is the
   same for every grid cell of the mesh, and the same bits in every run.  Tiles over slice ranges and pseudonormals inside the
   loop are not offered; the start from an unknown pose is ppp_register_mesh_global's (further down).
   ppp_get_mesh_trimmed_registration_terms evaluates once at T12 (NULL: the identity) and takes no step; its maps are that
   evaluation's.  rows, row, the maps and stats may be NULL (rows with row_cap = 0; the maps with any cap).  The whole chain -- per
   evaluation the grid walk, paid once, with the key, the top digit's histogram, two passes over the stored keys, the sums over
   the stored winners, the step -- is enqueued at once on h's stream with one wait at its end.  Neither call changes h's cloud,
   plan or stored results; the mesh gains its topology under _REJECT and is otherwise unchanged.
   PPP_ERR_ARG: m or mp NULL; rows NULL with row_cap > 0; ppp_register's parameter ranges; keep NaN, <= 0 or > 1; border neither
   of the two values; a T entry that is not finite; no cloud on h; a mesh on another device than h; shift < 16.
   PPP_ERR_UNSUPPORTED: a slice-range or a part handle. */
enum { PPP_MESH_BORDER_PAIR = 0, PPP_MESH_BORDER_REJECT = 1 };
typedef struct {
    ppp_trimmed_registration_params trim;   /* ppp_register_trimmed's: icp's four and keep in (0, 1] */
    int border;                             /* PPP_MESH_BORDER_PAIR (as ppp_register_mesh) or _REJECT */
} ppp_mesh_trimmed_registration_params;     /* defaults: ppp_default_trimmed_registration_params, PPP_MESH_BORDER_PAIR */
typedef struct {
    ppp_trimmed_registration_row trim;      /* row over the KEPT pairs, paired, trim_d2 */
    size_t on_border;                       /* candidates rejected on the border at row.T; 0 under _PAIR */
} ppp_mesh_trimmed_registration_row;
enum { PPP_MESH_TRIM_BORDER = 4 };          /* beside PPP_TRIM_KEPT .. PPP_TRIM_DROPPED, unchanged */

void ppp_default_mesh_trimmed_registration_params(ppp_mesh_trimmed_registration_params *mp);
int  ppp_get_mesh_trimmed_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_mesh_trimmed_registration_params *mp,
                                             const double *T12, ppp_mesh_trimmed_registration_row *row,
                                             unsigned char *status, float *d2, size_t cap, ppp_registration_stats *stats);
int  ppp_register_mesh_trimmed(ppp_handle h, ppp_trimesh m, const ppp_mesh_trimmed_registration_params *mp,
                               const double *T0_12, ppp_mesh_trimmed_registration_row *rows, size_t row_cap,
                               unsigned char *status, float *d2, size_t cap, ppp_registration_stats *stats);
/* T applied to the resident cloud: T12 (row-major 3 x 4, NULL: the identity) is rounded to float and every finite point
   becomes m0 x + (m1 y + (m2 z + m3)) per row, pcl::transformPointCloud's arithmetic; a point that is not finite passes
   unchanged.  The cloud has changed: bounds, plan, index and every stored result are withdrawn, as after ppp_trans2center.
   Does not set the alignment of ppp_trans2center.  PPP_ERR_ARG: no cloud, a slice-range or part handle (the preprocessing
   calls' refusals), a handle under ppp_trans2center, a T entry that is not finite. */
int  ppp_transform_cloud(ppp_handle h, const double *T12);
/* Global registration: the start ppp_register needs, from the two clouds alone.  Each cloud's
   principal frame -- mean and eigenvectors of its points' covariance -- is taken from ten order-free integer sums; two frames
   imply a rigid motion up to the 24 proper signed permutations G of the axes; a short coarse chain of ppp_register's iteration
   runs from each of them, side by side on a thinned scan, and the cheapest start seeds the fine chain.
     moments    n = cloud->size(); mn, mx = ppp_minmax; c[d] = ((double)mn[d] + (double)mx[d]) * 0.5, e = (double)mx - (double)mn,
                L = ((ex + ey) + ez) * 0.5; u = ((double)p - c) / L for every indexed (finite) point p; ms = min(40, 60 -
                clog2(max(2, n))); words[0] = the count, words[1 + d] = the sum of llrint(u_d 2^ms), words[4 ..] = the sums of
                llrint((u_d u_k) 2^ms) for dk = xx xy xz yy yz zz, in signed 64-bit integers
     frame      m_d = ((double)S1_d / (double)count) 2^-ms; C_dk = ((double)S2_dk / (double)count) 2^-ms - m_d m_k; the eigenpairs
                of C by 12 cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2): a pair with C_pq == 0 is skipped, else
                theta = (C_qq - C_pp) / (2 C_pq), t = sgn(theta) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1),
                s = t c; C_pp -= t C_pq, C_qq += t C_pq, C_pq = 0, the third index r: (C_rp, C_rq) <- (c C_rp - s C_rq,
                s C_rp + c C_rq), every row of V (from I) likewise.  Eigenvalues descending, a tie to the lower original column;
                each of the first two axes signed so that its component of largest magnitude is positive (the lowest index on a
                tie); the third axis = the cross product of the first two.  mean = c + L m (resident units), eigenvalues =
                (lambda L) L (mm^2), axes[3 d + k] = component d of axis k.
     starts     the G in this order: the identity; the half turns about axis 0, axis 1, axis 2 (diag(1,-1,-1), diag(-1,1,-1),
                diag(-1,-1,1)); the other 20, G's column k = sgn[k] e_perm[k], ascending in (perm[0], perm[1], perm[2], sgn[0],
                sgn[1], sgn[2]) with +1 before -1.  R_G = (V_ref G) V_scan^T, t_G = mean_ref - R_G mean_scan, every entry
                ((a0 b0) + a1 b1) + a2 b2.  candidates = 4 takes the first four: right where the three eigenvalues are well
                apart; 24 also covers axes that swap.
     coarse     the queries are the indexed points of h whose cloud index is a multiple of stride; from every start a chain of
                ppp_register with the parameters `coarse` on those queries alone, with ppp_register's c, Ln and shift for
                coarse.max_dist and n = cloud->size() of h (with stride 1 each chain IS ppp_register from that start)
     cost       of a start, from its last row: E + (queries - pairs) * llrint((double)md2 2^shift), md2 the float square of
                coarse.max_dist, in signed 64-bit integers: an unpaired query costs what the farthest pair could.  The smallest
                cost wins, a tie goes to the lower index.
     fine       ppp_register with the parameters `fine` from the winner's T: rows and stats.fine are that call's
   ppp_get_cloud_moments fills *frame for h's resident cloud (one kernel, one wait).  ppp_cloud_frame_from_moments and
   ppp_registration_starts are host only: no handle, no device.  ppp_register_global builds both handles' indices and ref's
   normal field where they are missing, takes both clouds' moments, enqueues coarse.iterations + 1 evaluations and
   coarse.iterations steps of all starts back to back on h's stream, waits once, then runs the fine chain.  cands receives the
   first min(cand_cap, candidates) starts' results, rows the first min(row_cap, steps + 1) rows of the fine chain; each may be
   NULL with a cap of 0; stats may be NULL.  stats.second_cost is the lowest cost among the starts whose T differs from the
   winner's (-1: none): close to winner_cost on a part that is ambiguous.  Neither cloud, plan nor any stored contact result
   changes.  h == ref is allowed.
   The defaults -- 24 candidates, stride 16, coarse 10 mm / 8 iterations / min_step 1e-3 / lock_eps 1e-9, fine =
   ppp_default_registration_params -- are a guess for parts of a few hundred millimetres.
   Limits: the two clouds must cover the same extent of the part -- the frames are those of the points, so a partial scan or a
   very uneven density moves the mean (ppp_voxel_down evens the density); a part whose relief is symmetric under one of the 24
   motions is ambiguous by nature: the tie rule answers and second_cost shows it.  No feature matching, no orientation test on
   the scan's own normals, no scale.
   PPP_ERR_ARG: ppp_register's refusals for `coarse` and for `fine`; gp NULL; candidates not 4 or 24; stride < 1; cands NULL
   with cand_cap > 0; no indexed point on either cloud; L == 0 on either cloud; no query left.  ppp_cloud_frame_from_moments:
   frame, words or c NULL, words[0] <= 0, ms outside [0, 62], L not finite and > 0.  ppp_registration_starts: a NULL
   argument, candidates not 4 or 24.  PPP_ERR_UNSUPPORTED when either handle is a slice-range handle or a part handle. */
typedef struct {
    size_t    count;            /* indexed (finite) points */
    int       ms;               /* the words' fixed point is 2^ms */
    double    c[3], L;          /* centre of the box and half the sum of its extents */
    long long words[10];        /* count, S1[x y z], S2[xx xy xz yy yz zz] */
    double    mean[3];          /* resident units */
    double    axes[9];          /* axes[3 d + k]: component d of axis k; a proper rotation */
    double    eigenvalues[3];   /* mm^2, descending */
} ppp_cloud_frame;

typedef struct {
    int candidates;                  /* 4 or 24 */
    int stride;                      /* >= 1: every stride-th cloud index is a query of the coarse stage */
    ppp_registration_params coarse;  /* the K chains side by side */
    ppp_registration_params fine;    /* the chain from the winner */
} ppp_global_registration_params;    /* defaults: 24, 16, (10, 8, 1e-3, 1e-9), (2, 30, 1e-6, 1e-9) */

typedef struct {
    int       index;                    /* of the start, in the order above */
    double    T0[12], T[12];            /* the start and where its chain ended */
    int       steps, converged, locked;
    size_t    pairs0, pairs;            /* at T0 and at T */
    long long E0, E;
    long long cost;
} ppp_registration_candidate;

typedef struct {
    ppp_registration_stats fine;        /* the fine chain's; fine.T is the result */
    ppp_cloud_frame scan, ref;
    size_t    queries;                  /* of the coarse stage */
    int       shift;                    /* the coarse stage's fixed point is 2^shift */
    int       candidates, winner;
    long long winner_cost, second_cost;
} ppp_global_registration_stats;

int  ppp_get_cloud_moments(ppp_handle h, ppp_cloud_frame *frame);
int  ppp_cloud_frame_from_moments(const long long *words10, int ms, const double *c3, double L, ppp_cloud_frame *frame);
int  ppp_registration_starts(const ppp_cloud_frame *scan, const ppp_cloud_frame *ref, int candidates, double *T12s);
void ppp_default_global_registration_params(ppp_global_registration_params *gp);
int  ppp_register_global(ppp_handle h, ppp_handle ref, const ppp_global_registration_params *gp,
                         ppp_registration_candidate *cands, size_t cand_cap, ppp_registration_row *rows, size_t row_cap,
                         ppp_global_registration_stats *stats);
/* Global registration to the triangle mesh itself: the start ppp_register_mesh needs, from the scan
   and the mesh alone -- no sampled cloud, no pitch, no normal field, no second handle.  ppp_register_global's rule with the
   reference side replaced: the mesh's frame is that of its SURFACE, from ten order-free integer sums over the indexed triangles
   (a vertex-weighted frame would be pulled towards the fillets of a CAD export, where the facets are small).
     moments    mn, mx = the mesh's box (ppp_trimesh_stats mn / mx, floats widened); c, L by ppp_get_cloud_moments' expressions;
                per indexed triangle, on the rotated resident floats of ppp_trimesh_create's frame widened to double:
                u_i = (p_i - c) / L for the three corners; N = (u1 - u0) x (u2 - u0), component by component e1y e2z - e1z e2y,
                e1z e2x - e1x e2z, e1x e2y - e1y e2x; a = sqrt((Nx Nx + Ny Ny) + Nz Nz) * 0.5; s = (u0 + u1) + u2;
                q_dk = ((u0_d u0_k + u1_d u1_k) + u2_d u2_k) + s_d s_k for dk = xx xy xz yy yz zz (a <= 2 sqrt 3, |q| <= 12);
                ms = min(40, 54 - clog2(max(2, n_tris))), n_tris the caller's triangle count; words[0] = W0 = the sum of
                llrint(a 2^ms), words[1 + d] = the sum of llrint((a s_d) 2^ms), words[4 ..] = the sums of llrint((a q_dk) 2^ms),
                in signed 64-bit integers.  The integrals of u_d and of u_d u_k over a triangle are a s_d / 3 and a q_dk / 12.
     frame      m_d = (double)S1_d / (3.0 * (double)W0); C_dk = (double)S2_dk / (12.0 * (double)W0) - m_d m_k; from there
                ppp_get_cloud_moments' frame unchanged: the Jacobi sweeps, the ordering, the signs, mean = c + L m,
                eigenvalues = (lambda L) L
     coarse     the starts of ppp_registration_starts(scan = h's point frame, ref = the mesh's area frame); the queries of
                ppp_register_global; from every start a chain of ppp_register_mesh with the parameters `coarse` on those queries,
                with ppp_register_mesh's c and Ln (the mesh's box) and shift (coarse.max_dist, n = cloud->size() of h): with
                stride 1 each chain IS ppp_register_mesh from that start, bit for bit
     cost, fine ppp_register_global's cost, winner, tie rule and second_cost; the fine chain is ppp_register_mesh with the
                parameters `fine` from the winner's T: rows and stats.fine are that call's
   ppp_trimesh_get_moments fills *frame for the mesh (one kernel and one wait on the mesh's own stream): ppp_cloud_frame is
   reused, with count = the indexed triangles and words[0] = W0, the area in fixed point -- NOT a count: for these words
   ppp_cloud_frame_from_moments is not the inverse, ppp_mesh_frame_from_moments is (host only; the words do not hold the
   triangle count, so it sets count = 0; every other member is ppp_trimesh_get_moments').  ppp_register_mesh_global builds h's
   slab index where it is missing, takes both frames, enqueues coarse.iterations + 1 evaluations (a search and a sum launch
   each) and coarse.iterations steps of all starts back to back on h's stream, waits once, then runs the fine chain.  stats.ref
   is the mesh's area frame, stats.scan the scan's point frame; cands, rows and stats otherwise as ppp_register_global fills
   them.  Neither the cloud, the plan, the mesh nor any stored result changes.  The same bits in every run, for every grid cell.
   Limits: the scan must cover the same extent as the mesh at an even density -- the scan's frame weighs points, the mesh's
   weighs area (ppp_voxel_down evens a scan); a closed mesh scanned from one side does not qualify; a part that is symmetric
   under one of the 24 motions is ambiguous, as for ppp_register_global; the fine chain has no robust weights: with a
   contaminated scan run ppp_register_mesh_robust from stats.fine.T.
   PPP_ERR_ARG: ppp_register_global's refusals for gp, `coarse`, `fine`, candidates, stride, cands and rows, and "no query
   left"; m NULL; a mesh on another device than h; shift < 16 for either parameter set; no indexed point on h or L == 0 on its
   cloud; W0 <= 0 (or L == 0) on the mesh; a start that is not finite.  ppp_trimesh_get_moments: m or frame NULL, W0 <= 0.
   ppp_mesh_frame_from_moments: a NULL argument, words[0] <= 0, ms outside [0, 62], L not finite and > 0.
   PPP_ERR_UNSUPPORTED: a slice-range or a part handle. */
int  ppp_trimesh_get_moments(ppp_trimesh m, ppp_cloud_frame *frame);
int  ppp_mesh_frame_from_moments(const long long *words10, int ms, const double *c3, double L, ppp_cloud_frame *frame);
int  ppp_register_mesh_global(ppp_handle h, ppp_trimesh m, const ppp_global_registration_params *gp,
                              ppp_registration_candidate *cands, size_t cand_cap, ppp_registration_row *rows, size_t row_cap,
                              ppp_global_registration_stats *stats);
/* The contact field of the resident cloud: for every cloud point i, compute_transform + Area2Cloud
   evaluated AT the point (query = its resident float coordinates, after the x1000 and any preprocessing).
     curv5[5*i..]  = what ppp_principal_curvatures_at returns for that query
     half_width[i] = the float r = (min x - max x) / 2 of the transformed contact ellipse: compute_coverage's comput_lan
                     (Path_Generation.cpp:464-467), the radius ppp_get_path_coverage marks with; NaN where Area2Cloud gives NaN
   for the first min(cap, n) points; either map may be NULL; stats may be NULL.  Both maps are bit-identical to the per-query
   forms: row i of curv5 is ppp_principal_curvatures_at on point i, half_width[i] is
   (ppp_area2cloud(p_i, 0).x - ppp_area2cloud(p_i, 1).x) / 2 in float -- the same neighbours in ascending (squared distance,
   cloud index), the same rank-order float sums, the same first-extremum fold.  Points dropped from the index (non-finite) have
   NaN in both maps and are not valid.  stats: n = cloud->size(), valid = points with a finite half width, narrow = valid points
   whose contact width 2|r| is below min_width (mm, the cloud's units; 0 when min_width <= 0), min_abs_r / max_abs_r (NaN when
   nothing is valid), sum_abs_r over the valid points by a fixed-order reduction (the same in every run), hist = valid points
   by floor(|r| / Tool_Radius * (PPP_CONTACT_BINS - 1)), clamped to the last bin.  min_width only sets what narrow counts: a
   pass over the stored map, not a recomputation.
   Needs a cloud and parameters, NOT a pass: it builds the slab index and the normal field if the handle has none, and a
   window-path handle stays on the window path.  Computed once per (cloud, parameters): later calls answer from the stored
   result until ppp_set_cloud*, a preprocessing call, or a ppp_set_params that changes tool_radius, depth, toolthickness,
   curvature_k, normal_radius or change_range.  A pass does not invalidate it, and it leaves the results of the three coverage
   calls alone.  Blocks until the results are on the host.  PPP_ERR_ARG without a cloud or with curvature_k outside [3, 64];
   PPP_ERR_UNSUPPORTED on a part handle (ppp_set_cloud_part) and on a slice-range handle (slice_begin / slice_end: its index
   holds a part of the cloud only: ppp_get_contact_field_tile below answers for the points such a handle owns). */
typedef struct {
    size_t n;            /* cloud->size() */
    size_t valid;        /* points with a finite half width */
    size_t narrow;       /* valid points whose contact width 2|r| is below the call's min_width (0 when min_width <= 0) */
    float  min_abs_r, max_abs_r;
    double sum_abs_r;    /* over the valid points, added in cloud index order on the host or by a fixed-order reduction */
    size_t hist[PPP_CONTACT_BINS]; /* valid points by floor(|r| / Tool_Radius * (PPP_CONTACT_BINS - 1)), clamped */
} ppp_contact_field_stats;
int ppp_get_contact_field(ppp_handle h, float *curv5, float *half_width, size_t cap, float min_width,
                          ppp_contact_field_stats *stats);
/* Connected regions of selected cloud points: WHERE the points a contact query singles out lie, in
   how many pieces, and how large each piece is.  source picks the points: those ppp_get_path_coverage does not flag, those
   with last_slice > first_slice in ppp_get_path_contacts, the valid points of ppp_get_contact_field whose contact width 2|r| is
   below threshold (mm; threshold is read for this source only), or the caller's mask.  Points dropped from the index
   (non-finite) are never selected, whatever the source or the mask says.  Two selected points are LINKED when their squared
   distance, in float as every radius search of the engine computes it (((dx*dx) + dy*dy) + dz*dz), is <= link_radius *
   link_radius (the float product); link_radius <= 0 means the handle's normal_radius.  A region is a connected component of
   that graph.
     labels[i]  = the region's label for a selected point i, -1 otherwise, for the first min(cap, n) points
     regions[]  = the regions in ascending label, the first min(region_cap, stats->regions) of them
   A region's label is the smallest cloud index in it: its name, the same in every run.  count is exact; mn / mx are the exact
   float minima / maxima of its points; centroid[c] = (the sum over its points of llrint((double)p[c] * 2^20), taken in 64-bit
   integers) / count / 2^20 in double -- an integer sum has no order, so labels, rows and stats are the same bits in every run
   and on every fresh handle.  If max |coordinate| * 2^20 * selected could reach 2^62, all centroids are NaN and nothing else
   changes.  stats: n = cloud->size(), selected, regions, singletons = regions of one point, largest = the largest count.
   Every output pointer may be NULL; cap = 0 / region_cap = 0 is the size query.
   Builds, reuses and refuses like its source: UNCOVERED / OVERLAP need a finished pass and go through ppp_get_path_coverage /
   ppp_get_path_contacts (building that result if the handle does not hold it, leaving it untouched if it does); NARROW needs a
   cloud and parameters only, as ppp_get_contact_field; MASK needs a cloud only (it builds the slab index if the handle has
   none).  A window-path handle stays on the window path.  The result is kept per (source, threshold, link radius, the source's
   result): a repeated call launches nothing; a MASK call always recomputes.  No region call invalidates or recomputes one of
   the four contact results.  Blocks until the results are on the host.
   PPP_ERR_ARG: no cloud; UNCOVERED / OVERLAP before any pass; an unknown source; MASK with mask == NULL; NARROW with a threshold
   that is not a positive finite number; a NaN or infinite link_radius; curvature_k outside [3, 64] where the source refuses it.
   PPP_ERR_UNSUPPORTED on a slice-range handle (slice_begin / slice_end) and on a part handle (ppp_set_cloud_part): a region does
   not stop at a range border: ppp_get_regions_tile and ppp_merge_region_tiles below tile the regions over ranges.  The pass's own error if it failed.  PPP_ERR_CAPACITY
   if a walk of the union-find reaches its trip cap (no sound input does). */
enum { PPP_REGIONS_UNCOVERED = 0,  /* points ppp_get_path_coverage does not flag (indexed points only)            */
       PPP_REGIONS_OVERLAP   = 1,  /* points with last_slice > first_slice in ppp_get_path_contacts               */
       PPP_REGIONS_NARROW    = 2,  /* valid points of ppp_get_contact_field with 2|r| < threshold (mm)            */
       PPP_REGIONS_MASK      = 3   /* the caller's mask: n bytes on the host, non-zero = selected                 */ };
typedef struct {
    int          label;        /* the smallest cloud index in the region: its name, the same in every run */
    unsigned int count;        /* points in it */
    float        mn[3], mx[3]; /* bounding box, resident coordinates (mm after ChangeRange) */
    double       centroid[3];  /* fixed-point mean (see above) */
} ppp_region;
typedef struct { size_t n, selected, regions, singletons, largest; } ppp_region_stats;
int ppp_get_regions(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius,
                    int *labels, size_t cap, ppp_region *regions, size_t region_cap, ppp_region_stats *stats);
/* ---- the contact field and the regions tiled over slice ranges ----
   OWNERSHIP.  The walk of a pass is px[0 .. S), ascending.  cut(0) = -INFINITY, cut(S) = +INFINITY, and for 0 < s < S
   cut(s) = ((float)px[s-1] + (float)px[s]) * 0.5f in float.  A handle with the slice range [sb, se) OWNS the indexed points
   with cut(sb) <= x < cut(se), x in planner units; a whole-cloud handle owns every indexed point; non-finite points are owned
   by no one.  Ranges that tile [0, S) therefore partition the indexed points exactly.  ppp_range_owned: host arithmetic only,
   beside ppp_range_interval: own_lo = cut(sb), own_hi = cut(se) for p's range on a cloud with these x bounds (an empty range:
   own_lo = +INFINITY, own_hi = -INFINITY). */
int ppp_range_owned(const ppp_params *p, float min_x, float max_x, float *own_lo, float *own_hi);
/* The contact field of the points a handle owns: ppp_get_contact_field's maps, evaluated for every indexed point with x in
   [own_lo - halo, own_hi + halo] (halo >= 0 mm, finite; 0 for the owned points alone).
     owned[i]      = 1 for an owned point, 2 for an evaluated halo point, 0 otherwise
     curv5, half_width: by whole-cloud point index, for the first min(cap, n) points; NaN for every point that was not
                     evaluated.  Rows of evaluated points are bit-identical to ppp_get_contact_field on a whole-cloud handle
                     with the same cloud and parameters (the same slab grid and point order, the same neighbours: B.28, B.37).
   stats cover the OWNED points only: ppp_contact_field_stats' fields, then owned / evaluated (point counts) and the owned
   interval.  Over ranges that tile the walk valid, narrow and every hist[b] add up to the whole field's; min_abs_r / max_abs_r
   are the minimum / maximum over the tiles; sum_abs_r is a fixed-order sum inside the tile.
   Every search of an evaluated point -- its k nearest neighbours (and a full k of them) and the normal_radius neighbourhood of
   every neighbour read -- must lie inside the handle's indexed interval unless that reaches the cloud's end: where one does
   not, the call fails with PPP_ERR_CAPACITY (raise range_margin); it is never answered with fewer points.
   Needs a cloud and parameters, not a pass; builds the slab index and the normal field as ppp_get_contact_field does.  The
   result is kept per (cloud, contact parameters, range, halo): a repeated call launches nothing, a new min_width runs the
   statistics alone.  On a whole-cloud handle the call equals ppp_get_contact_field with owned = 1 on the indexed points.
   PPP_ERR_ARG: no cloud, curvature_k outside [3, 64], a negative or non-finite halo; PPP_ERR_UNSUPPORTED on a part handle
   (ppp_set_cloud_part). */
typedef struct {
    size_t n, valid, narrow;           /* as ppp_contact_field_stats, over the owned points */
    float  min_abs_r, max_abs_r;
    double sum_abs_r;
    size_t hist[PPP_CONTACT_BINS];
    size_t owned, evaluated;           /* owned points; owned + halo points */
    float  own_lo, own_hi;             /* the owned interval [own_lo, own_hi) */
} ppp_contact_field_tile_stats;
int ppp_get_contact_field_tile(ppp_handle h, float *curv5, float *half_width, unsigned char *owned, size_t cap, float halo,
                               float min_width, ppp_contact_field_tile_stats *stats);
/* The regions of one tile: the connected components (ppp_get_regions' link) of the selected indexed points with x in
   [own_lo - link, own_hi + link], link = the link radius: the owned points and a halo of one link radius, which holds every
   point an owned point can be linked to.  source: PPP_REGIONS_MASK (the caller's mask over the WHOLE cloud, by cloud index) or
   PPP_REGIONS_NARROW (through ppp_get_contact_field_tile with halo = link).  UNCOVERED / OVERLAP are refused with
   PPP_ERR_UNSUPPORTED: a range's coverage flags know its own slices' balls only -- OR the ranges' flags
   (ppp_get_path_coverage) and pass the complement as a mask.
     labels[i] = the tile-local label of an OWNED selected point, -1 otherwise: the smallest cloud index of its tile component,
                 halo points included
     parts[]   = one row per tile component with at least one owned point, in ascending label: count, mn / mx and the three
                 64-bit fixed-point sums of ppp_region's centroid (fsum[c] = the sum of llrint((double)p[c] * 2^20)), all over
                 its OWNED points
     halos[]   = one entry per evaluated halo point that is selected and lies in such a component, in ascending cloud index
   stats: n = cloud->size(), selected = owned selected points, parts, halo_points, max_abs_coord = the largest |coordinate|
   bound of the cloud (what the centroid's overflow rule reads), the owned interval.  Every output pointer may be NULL;
   cap = 0 / part_cap = 0 / halo_cap = 0 is the size query; a MASK call always recomputes.  The call replaces the result a
   ppp_get_regions call left on the handle (that call then computes again).
   PPP_ERR_CAPACITY (raise range_margin) when [own_lo - link, own_hi + link] leaves the indexed interval at a side that is not
   the cloud's end, and for the union-find's trip cap; PPP_ERR_UNSUPPORTED on a part handle; PPP_ERR_ARG as ppp_get_regions. */
typedef struct { int cloud_index, label; } ppp_region_halo;
typedef struct {
    int          label;
    unsigned int count;        /* owned points */
    float        mn[3], mx[3]; /* over the owned points */
    long long    fsum[3];      /* over the owned points */
} ppp_region_part;
typedef struct {
    size_t n, selected, parts, halo_points;
    double max_abs_coord;
    float  own_lo, own_hi;
} ppp_region_tile_stats;
int ppp_get_regions_tile(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius,
                         int *labels, size_t cap, ppp_region_part *parts, size_t part_cap, ppp_region_halo *halos, size_t halo_cap,
                         ppp_region_tile_stats *stats);
/* Merges the tiles of ranges that tile the walk (host only: no handle, no device).  tile t gives labels[t] (n ints), parts[t]
   (stats[t].parts rows), halos[t] (stats[t].halo_points entries) and stats[t] as ppp_get_regions_tile returned them.  A
   union-find over (tile, label): every halo entry {p, a} of tile t unites (t, a) with (u, labels[u][p]), u the tile that owns
   p.  A merged region's label is the smallest part label in it, count and fsum are integer sums, mn / mx minima and maxima,
   the centroid comes from the summed fsum as ppp_region's, NaN by its rule with the merged selected count and the largest
   max_abs_coord.  out_labels (the first min(cap, n)), regions (ascending label, the first min(region_cap, regions)) and
   out_stats are the same bits as ppp_get_regions on a whole-cloud handle with that mask or threshold and link radius.
   PPP_ERR_ARG: a point two tiles own, a halo entry whose point no tile owns, tiles that disagree on n, a label without its
   part row. */
int ppp_merge_region_tiles(size_t tiles, const int *const *labels, const ppp_region_part *const *parts,
                           const ppp_region_halo *const *halos, const ppp_region_tile_stats *stats,
                           int *out_labels, size_t cap, ppp_region *regions, size_t region_cap, ppp_region_stats *out_stats);
/* ---- the deviation map tiled over slice ranges ----
   ppp_get_deviation for the points a handle owns.  h: a slice-range handle of the scan (it holds the whole cloud and indexes
   its range plus range_margin), or a whole-cloud handle, which owns every indexed point; ownership is ppp_range_owned's rule
   and no other.  ref: a whole-cloud handle of the reference, or a slice-range handle of it.  The two clouds are registered in
   one frame, so the scan's cuts are x coordinates of the reference as well.
     halo      mm, finite, >= max_dist + smooth_radius (the float sum; so max_dist must be finite): how far beyond the owned
               interval [own_lo, own_hi) the call may have to look -- a partner lies within max_dist of a point that is evaluated
               because it lies within smooth_radius of an owned one.  W(r) = [nextbelow(own_lo - 1.0001f r), nextabove(own_hi +
               1.0001f r)] in float: the interval widened by r with room for the roundings of a float distance test.  ref must
               index W(halo + ref's normal_radius) (a partner's normal reads that neighbourhood) unless its index reaches the
               reference's end on that side; h must index W(smooth_radius) likewise, and evaluates the points in it.  Both are
               decided on the host from the two handles' plans, before any launch: no index is built and no kernel runs on
               either handle for a call that is refused (a handle plans when its cloud is set; only one whose parameters
               changed since makes its plan first).  What does not reach is PPP_ERR_ARG, never a silent TOO_FAR.
     maps      by cloud index of h, the first min(cap, n) entries.  For every OWNED point all five hold exactly the bits
               ppp_get_deviation gives for the same two clouds on whole-cloud handles with the same dp: the slab grids and point
               orders are the whole clouds', a reference range handle's points carry their whole-cloud indices (the tie rule and
               ref_index are the whole reference's), and the smoothing sums integers.  Every other point has status
               PPP_DEV_DROPPED, ref_index -1, deviation and smoothed the NaN, target +0, and owned[i] = 0 (owned[i] = 1 for an
               owned point).  The halo points the smoothing needed are evaluated, enter the owned points' sums and are reported
               nowhere.
     part      over the OWNED points: n = cloud->size() of h; owned, and evaluated = owned + halo points; matched, too_far,
               no_normal (an owned point is indexed: never DROPPED); proud, below; min_dev / max_dev over v (NaN when matched ==
               0); fix_sum = the integer sum of llrint(v_i 2^24); max_dist2; the owned interval; sum_parts = the number of
               contiguous parts ppp_get_deviation's fixed-order sums cut a map of n entries into on h's device.
   Needs clouds and parameters, not a pass; builds what ppp_get_deviation builds, waits and blocks as it does, keeps nothing and
   changes nothing stored on either handle; a window-path handle stays on the window path.  Every output may be NULL.
   PPP_ERR_ARG as ppp_get_deviation, and: max_dist not finite, halo below max_dist + smooth_radius or not finite, the two range
   conditions above.  PPP_ERR_UNSUPPORTED when either handle is a part handle (ppp_set_cloud_part). */
typedef struct {
    size_t n, owned, evaluated;
    size_t matched, too_far, no_normal;  /* the owned points by status */
    size_t proud, below;
    double min_dev, max_dev;             /* over v of the owned matched points; NaN when matched == 0 */
    long long fix_sum;                   /* the sum of llrint(v 2^24) over them */
    float  max_dist2;                    /* NaN when matched == 0 */
    float  own_lo, own_hi;               /* the owned interval [own_lo, own_hi) */
    int    sum_parts;
} ppp_deviation_tile_stats;
int ppp_get_deviation_tile(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp, float halo,
                           double *deviation, double *smoothed, int *ref_index, unsigned char *status,
                           double *target, unsigned char *owned, size_t cap, ppp_deviation_tile_stats *part);
/* Merges the parts of tiles whose ranges tile the walk into ppp_get_deviation's statistics of the whole cloud, bit for bit
   (host only: no handle, no device).  tile t gives parts[t] and its maps as ppp_get_deviation_tile returned them, n entries
   each: v[t] (its smoothed map: the deviation where smooth_radius == 0), status[t], target[t], owned[t].  The counts, fix_sum
   and the extrema merge by addition and minimum / maximum; dropped = n - the owned points.  hist depends on the span of the
   WHOLE cloud, and rms_dev / target_sum are sums of doubles in ppp_removal_stats' fixed order -- sum_parts contiguous parts of
   the map, inside a part 256 strided shares in index order and a fixed tree over them, the parts in order --, which no tile can
   add up on its own: the merge computes these three here, on the host, from the union of the owned entries in that order.
   PPP_ERR_ARG: a NULL argument, tiles that disagree on n or sum_parts, a point two tiles own, a part that is not its maps'. */
int ppp_merge_deviation_tiles(size_t tiles, const ppp_deviation_tile_stats *parts, const double *const *v,
                              const unsigned char *const *status, const double *const *target,
                              const unsigned char *const *owned, ppp_deviation_stats *stats);
/* ---- registration of a scan held as slice-range tiles ----
   ppp_register's evaluation is 29 signed 64-bit integer sums over the scan's pairs; integer sums have no order and the owned
   sets of ranges that tile the walk partition the indexed points (ppp_range_owned), so the whole cloud's words are the
   word-by-word sum of the tiles' words, bit for bit.  The solve and the step are the device chain's own routines, run on the
   host.  Nothing here approximates.
   ppp_get_registration_terms_tile (B.88-B.90): ppp_get_registration_terms over the points h owns.  h: a slice-range handle of
   the scan (it holds the whole cloud), or a whole-cloud handle, which owns every indexed point; ownership goes by the
   resident, unmoved x.  ref: a whole-cloud or a slice-range handle of the reference.  centre, length and shift are the WHOLE
   clouds': the reference's bounds (a range handle keeps the whole cloud's, cached with its plan) and n = cloud->size() of h.
     row       T = T12 (NULL: the identity), pairs / A / b / E over the owned points' pairs, locked 63, step2 NaN
     part      owned = the indexed points h owns, evaluated = the index positions visited (the slabs that meet the owned
               interval), the owned interval [own_lo, own_hi), n, shift, centre, length: what the merge and the step take
     range     a query is moved by T, so the two plans cannot decide what the reference must index.  With reach = 1.0001f *
               (max_dist + ref's normal_radius), the float sum: for every owned query with a finite moved x', the interval
               [nextbelow(x' - reach), nextabove(x' + reach)] must lie inside ref's indexed x interval, a side where that
               interval ends at the reference cloud's own end exempt.  One query that does not: PPP_ERR_CAPACITY (raise
               range_margin); a call is never answered with fewer pairs.  The test is conservative: it refuses even where no
               pair would have been found.  A whole-cloud reference never refuses.
   Builds what ppp_get_registration_terms builds, keeps nothing, changes no plan, path or stored result of either handle.
   PPP_ERR_ARG as ppp_get_registration_terms (B.72); PPP_ERR_UNSUPPORTED when either handle is a part handle
   (ppp_set_cloud_part).  h == ref is allowed.  row and part may be NULL.
   ppp_merge_registration_terms (B.91; host only): the 29 words and pairs add as signed 64-bit integers (two's complement),
   owned and evaluated add, the owned interval is the hull; out_row->T = T12 (NULL: the identity), locked 63, step2 NaN.
   out_part may be NULL.  PPP_ERR_ARG: rows, parts or out_row NULL, count == 0, parts that disagree on n, shift, centre or
   length (compared bit for bit), owned intervals that overlap (equal ends that meet are fine: ownership is half-open; an
   interval with own_lo >= own_hi is empty and overlaps nothing).
   ppp_registration_step (B.92; host only): the step ppp_register takes from an evaluation.  T12 (NULL: row->T) is the
   transform the row was taken at, part gives centre and length.  Returns PPP_STEP_TAKEN with T12_out, *locked (the mask) and
   *step2; or, with T12_out = T12, *locked = 63 and *step2 = NaN, PPP_STEP_FEW_PAIRS (pairs < 6), PPP_STEP_STATIONARY (all six b
   zero: T is a stationary point, ppp_register ends converged) or PPP_STEP_ALL_LOCKED (the pivot rule locked all six
   unknowns).  locked and step2 may be NULL.  PPP_ERR_ARG: row, part or T12_out NULL, lock_eps outside (0, 1), part->length not
   finite and > 0.
   ppp_register_tiles (B.93, B.94): ppp_register's loop over tiles.  hs[i] holds the scan with range i, refs[i] is the
   reference handle of tile i (the same whole-cloud handle may stand in every slot); tiles may sit on different devices, a tile
   and its own reference on the same one.  Each reference's index and normal field are built once, before the loop.  Per
   evaluation T goes to every tile's device, every tile's evaluation is enqueued on its own handle's stream, the words come back
   with one asynchronous copy per tile, the host waits for all tiles, merges, steps and records the row: one host round trip
   per evaluation, where ppp_register has none.  For ranges that tile the walk T, every row (words, locked, step2) and every
   field of stats->reg are the bits of ppp_register on whole-cloud handles with the same parameters and T0.  A tile's error
   ends the loop and is returned (the text on that tile's handle), with the tile's index in stats->failed_tile (-1 otherwise).
   PPP_ERR_ARG: hs, refs or params NULL, count == 0, a NULL handle, a handle twice in hs, rows NULL with row_cap > 0, and
   ppp_register's own. */
typedef struct {
    size_t owned, evaluated;   /* indexed points owned; index positions visited */
    float  own_lo, own_hi;     /* the owned interval [own_lo, own_hi) */
    size_t n;                  /* cloud->size() of the whole scan */
    int    shift;              /* the fixed point is 2^shift */
    double centre[3], length;  /* c and Ln of ppp_register, from the whole reference */
} ppp_registration_part;
typedef struct {
    ppp_registration_stats reg; /* ppp_register's statistics */
    int failed_tile;            /* the tile whose error ended the loop; -1: none */
} ppp_register_tiles_stats;
enum { PPP_STEP_TAKEN = 0, PPP_STEP_FEW_PAIRS = 1, PPP_STEP_STATIONARY = 2, PPP_STEP_ALL_LOCKED = 3 };
int ppp_get_registration_terms_tile(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T12,
                                    ppp_registration_row *row, ppp_registration_part *part);
int ppp_merge_registration_terms(const ppp_registration_row *rows, const ppp_registration_part *parts, size_t count,
                                 const double *T12, ppp_registration_row *out_row, ppp_registration_part *out_part);
int ppp_registration_step(const ppp_registration_row *row, const ppp_registration_part *part, double lock_eps,
                          const double *T12, double *T12_out, int *locked, double *step2);
int ppp_register_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count, const ppp_registration_params *rp,
                       const double *T0_12, ppp_registration_row *rows, size_t row_cap, ppp_register_tiles_stats *stats);
/* ---- trimmed registration of a scan held as slice-range tiles ----
   Every quantity of ppp_register_trimmed's evaluation is an integer histogram or an integer sum: pairs and keys are a point's
   own, the cut is a rank statistic of the union of the keys, the 29 words add.  So the tiles merge exactly, at the price of
   four host waits per evaluation.
   ppp_trim_select (B.95; host only): the device's selection rule on a histogram of `bins` counts: *bin = the first bin whose
   running count reaches rank (1-based), *rank_in_bin = rank minus the counts below that bin (>= 1).  rank 0 or a rank above
   the total finds nothing: *bin = 0 and *rank_in_bin = 0.  PPP_ERR_ARG: a NULL argument.
   ppp_trim_rank (B.96; host only): k = (size_t)ceil(keep * (double)paired), one double product and one ceil, clamped to
   [1, paired]; 0 when paired == 0.
   ppp_register_trimmed_tiles (B.97-B.100): ppp_register_trimmed's loop over tiles.  hs, refs and count are
   ppp_register_tiles's, with its rules; each reference's index and normal field are built once, before the loop.  An
   evaluation is four passes, each enqueued on every tile's own stream with one small asynchronous copy back per tile and one
   wait per tile: (1) the search, which stores an owned point's partner and key and counts the keys' top 11 bits; the host
   adds the tiles' histograms bin by bin, takes paired = their total and k = ppp_trim_rank(keep, paired) -- never a tile's own
   count --, selects the bin (ppp_trim_select) and sends every tile the merged prefix; (2), (3) the middle 11 and the low 10
   bits of the stored keys that carry the merged prefix, merged and selected likewise, which gives tau; (4) the 29 words over
   key <= tau, merged as ppp_merge_registration_terms does.  The histograms come back once each: 8 KB, 8 KB, 4 KB.  paired == 0
   ends the evaluation behind pass (1): trim_d2 = 0x7fc00000, kept 0.  The step is ppp_registration_step's.  For ranges that
   tile the walk T, every row (the 29 words, pairs = kept, locked, step2, paired, trim_d2), every field of stats->reg and each
   owned point's status / d2 are the bits of ppp_register_trimmed on whole-cloud handles with the same parameters and T0.
     status, d2, owned   arrays of `count` per-tile pointers; the array or any entry may be NULL.  Each holds the first
                         min(cap, n) entries by cloud index of tile i's maps of the LAST evaluation: an indexed point the tile
                         owns has owned 1 and its status / d2 as ppp_register_trimmed gives them; every other entry has
                         owned 0, PPP_TRIM_DROPPED and NaN (0x7fc00000).  The owned maps of ranges that tile the walk
                         partition the indexed points; a point no tile owns is not finite.
   A tile's error ends the loop and is returned (the text on that tile's handle), with its index in stats->failed_tile (-1
   otherwise).  PPP_ERR_ARG: ppp_register_tiles's refusals; tp NULL; keep NaN, <= 0 or > 1.  PPP_ERR_CAPACITY (raise
   range_margin): a moved owned query whose reach leaves a slice-range reference's index, by ppp_get_registration_terms_tile's
   test; such a call is never answered with fewer pairs.  PPP_ERR_UNSUPPORTED: a part handle.  Neither handle's cloud, plan
   or stored result changes; nothing is kept. */
int    ppp_trim_select(const unsigned int *hist, size_t bins, size_t rank, unsigned int *bin, size_t *rank_in_bin);
size_t ppp_trim_rank(double keep, size_t paired);
int    ppp_register_trimmed_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count,
                                  const ppp_trimmed_registration_params *tp, const double *T0_12,
                                  ppp_trimmed_registration_row *rows, size_t row_cap,
                                  unsigned char *const *status, float *const *d2, unsigned char *const *owned, size_t cap,
                                  ppp_register_tiles_stats *stats);
/* ---- robust registration of a scan held as slice-range tiles ----
   Everything ppp_register_robust's evaluation needs merges exactly over tiles: a pair, its residual r and its key (the bits of
   (float)fabs(r)) are a point's own, the median is a rank statistic of the union of the keys -- the three digit histograms add
   bin by bin --, sigma and the cut cs follow from the merged tau by two double multiplications and a max, the weight is a
   function of a point's own r and the merged cs, and the 30 words are integer sums.  Nothing is approximated; the price is
   ppp_register_trimmed_tiles's four host waits per evaluation.
   ppp_robust_sigma (B.102's rule; host only): sigma = max(1.4826 * m, sigma_min), m the double of the float whose bits are
   median_bits; none != 0 (an evaluation without a pair): the double quiet NaN 0x7ff8000000000000.  It is the routine the
   kernels compile, so a caller who reduces the histograms across ranks itself makes the scale as the library does.
   ppp_robust_weight (B.103's rule; host only): tune == +INFINITY: 1.  cs == 0: 1 where r == 0, else 0.  Otherwise
   u = r / cs, v = 1 - u * u, fabs(u) < 1 ? v * v : 0, one rounding per written operation.  Neither needs a device or a handle.
   ppp_register_robust_tiles (B.106-B.110): ppp_register_robust's loop over tiles.  hs, refs and count are
   ppp_register_tiles's, with its rules; each reference's index and normal field are built once, before the loop.  An
   evaluation is four passes, each enqueued on every tile's own stream with one small asynchronous copy back per tile and one
   wait per tile: (1) the search, which stores an owned point's partner, r and key and counts the keys' top 11 bits; the host
   adds the tiles' histograms bin by bin, takes paired = their total and k = ppp_trim_rank(0.5, paired) -- never a tile's own
   count --, selects the bin (ppp_trim_select) and sends every tile the merged prefix; (2), (3) the middle 11 and the low 10
   bits of the stored keys that carry the merged prefix, merged and selected likewise, which gives tau; (4) tau, 4 bytes, goes
   to every tile, whose kernel makes sigma = ppp_robust_sigma(tau, 0, sigma_min) and cs = tune * sigma itself and adds the 30
   words over its owned pairs; 240 bytes come back per tile and merge as ppp_merge_registration_terms merges 29.  paired == 0
   ends the evaluation behind pass (1): median_abs = 0x7fc00000, sigma the double quiet NaN, used 0, no step.  The step is
   ppp_registration_step's on a row that carries used in pairs ("fewer than 6 pairs" is used < 6); the row that is recorded
   carries paired.  For ranges that tile the walk T, every row (the 30 words, pairs = paired, used, weight_sum, median_abs,
   sigma, locked, step2), every field of stats->reg (ppp_register_robust's: pairs_* = paired, rms_* = sqrt((double)E /
   (double)weight_sum), NaN when weight_sum == 0) and each owned point's status / weight / residual are the bits of
   ppp_register_robust on whole-cloud handles with the same parameters and T0; tune == +INFINITY gives ppp_register_tiles's rows.
     status, weight, residual, owned   arrays of `count` per-tile pointers; the array or any entry may be NULL.  Each holds
                         the first min(cap, n) entries by cloud index of tile i's maps of the LAST evaluation: an indexed
                         point the tile owns has owned 1 and its status / (float)w / r as ppp_register_robust gives them;
                         every other entry has owned 0, PPP_ROBUST_DROPPED, the float NaN 0x7fc00000 and the double NaN
                         0x7ff8000000000000.  The owned maps of ranges that tile the walk partition the indexed points.
   A tile's error ends the loop and is returned (the text on that tile's handle), with its index in stats->failed_tile (-1
   otherwise).  PPP_ERR_ARG: ppp_register_tiles's refusals; bp NULL; tune NaN or <= 0 (+INFINITY is allowed); sigma_min not
   finite or < 0.  PPP_ERR_CAPACITY (raise range_margin): a moved owned query whose reach leaves a slice-range reference's
   index, by ppp_get_registration_terms_tile's test; such a call is never answered with fewer pairs.  PPP_ERR_UNSUPPORTED: a
   part handle.  Neither handle's cloud, plan or stored result changes; nothing is kept. */
double ppp_robust_sigma(unsigned int median_bits, int none, double sigma_min);
double ppp_robust_weight(double r, double cs, double tune);
int    ppp_register_robust_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count,
                                 const ppp_robust_registration_params *bp, const double *T0_12,
                                 ppp_robust_registration_row *rows, size_t row_cap,
                                 unsigned char *const *status, float *const *weight, double *const *residual,
                                 unsigned char *const *owned, size_t cap,
                                 ppp_register_tiles_stats *stats);
/* ---- the mesh calls for the points a handle owns ----
   The exact deviation (unsigned and signed) and the plain point-to-plane registration against a resident triangle mesh, for a
   scan held as slice-range tiles.  The mesh is resident whole on every device, so nothing on the reference's side needs a halo,
   a range condition or a refusal: only the scan's own smoothing reaches across a seam.
   ppp_get_mesh_deviation_tile / ppp_get_mesh_signed_deviation_tile (B.144-B.146): ppp_get_mesh_deviation /
   ppp_get_mesh_signed_deviation for the points h owns.  h: a slice-range handle of the scan (it holds the whole cloud and
   indexes its range plus range_margin), or a whole-cloud handle, which owns every indexed point; ownership is ppp_range_owned's
   rule and no other.  m: a mesh on h's device.  There is no halo argument: the call evaluates the scan's indexed points in
   W(smooth_radius), ppp_get_deviation_tile's widened interval, and h must index it unless its index reaches the cloud's end on
   that side -- decided on the host from h's plan, before any launch: PPP_ERR_ARG, never a silent change of a smoothed value.
     maps      by cloud index of h, the first min(cap, n) entries.  For every OWNED point every map holds exactly the bits the
               whole-cloud call gives for the same cloud on a whole-cloud handle with the same dp and a mesh of the same
               triangles (whatever its cell).  Every other point has status PPP_DEV_DROPPED, tri_index -1, region and feature
               255, deviation / signed_distance, smoothed and distance the NaN, target +0, flags 0 and owned[i] = 0.  The halo
               points the smoothing needed are evaluated, enter the owned points' integer sums and are reported nowhere.
     part      dev: ppp_get_deviation_tile's part over the owned points (evaluated = owned + halo points; a tile's launches
               cover the index positions of the slabs that meet W(smooth_radius), not n); on_face, on_edge, on_vertex and
               max_distance (NaN when matched == 0) over the owned matched points; the signed call adds on_border, irregular,
               fallback, negative and positive over them.
   Needs a cloud and parameters, not a pass; builds what the whole-cloud call builds (the signed call the mesh's topology where
   it is missing), keeps nothing and changes nothing stored on the handle.  Every output may be NULL.  PPP_ERR_ARG as the
   whole-cloud call, and the range condition above; PPP_ERR_UNSUPPORTED for a part handle (ppp_set_cloud_part).
   ppp_merge_mesh_deviation_tiles / ppp_merge_mesh_signed_deviation_tiles (B.147; host only, no handle): the whole cloud's
   ppp_mesh_deviation_stats / ppp_mesh_signed_deviation_stats, bit for bit, from the parts and maps of ranges that tile the walk.
   dev is ppp_merge_deviation_tiles' result on the parts' dev and the maps v (the smoothed map: the deviation or signed distance
   where smooth_radius == 0), status, target, owned; the counts add; max_distance is the maximum, NaN when nothing matched.
   PPP_ERR_ARG: what ppp_merge_deviation_tiles refuses (a point two tiles own among it), a part whose counts by region do not
   add up to its matched points, a max_distance that is negative or NaN on a part that matched.
   ppp_get_mesh_registration_terms_tile (B.148): ppp_get_mesh_registration_terms over the points h owns; ownership goes by the
   resident, unmoved x.  row: T = T12 (NULL: the identity), pairs / A / b / E over the owned points' pairs, locked 63, step2 NaN.
   part: ppp_get_registration_terms_tile's, with centre and length from the mesh's box and shift from n = cloud->size() of h, as
   ppp_register_mesh defines them.  There is no range condition and no PPP_ERR_CAPACITY: the mesh is whole.  The rows and parts
   go through ppp_merge_registration_terms and ppp_registration_step unchanged.
   ppp_register_mesh_tiles (B.149): ppp_register_mesh's loop over tiles, ppp_register_tiles's in shape: hs[i] holds the scan
   with range i, ms[i] is the mesh on hs[i]'s device (one mesh may stand in every slot when all tiles share a device); meshes in
   different slots must agree on triangles, indexed and the box, bit for bit.  Per evaluation T goes to every tile's device,
   the search and the sum are enqueued on every tile's own stream, the words come back with one asynchronous copy per tile, the
   host waits for all tiles, merges, steps and records the row: one host round trip per evaluation, where ppp_register_mesh has
   none.  For ranges that tile the walk T, every row and every field of stats->reg are the bits of ppp_register_mesh on a
   whole-cloud handle with the same parameters and T0.  A tile's error ends the loop and is returned (the text on that tile's
   handle), with its index in stats->failed_tile (-1 otherwise).  PPP_ERR_ARG: ppp_register_tiles's and ppp_register_mesh's
   refusals, a NULL mesh, meshes that disagree.  PPP_ERR_UNSUPPORTED: a part handle.
   The whole-cloud calls still refuse a slice-range handle; the robust and trimmed mesh loops have no tiled form yet. */
typedef struct {
    ppp_deviation_tile_stats dev;
    size_t on_face, on_edge, on_vertex;  /* the owned matched points by region */
    double max_distance;                 /* over them; NaN when dev.matched == 0 */
} ppp_mesh_deviation_tile_stats;
typedef struct {
    ppp_mesh_deviation_tile_stats mesh;
    size_t on_border, irregular, fallback, negative, positive;
} ppp_mesh_signed_deviation_tile_stats;
int ppp_get_mesh_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp,
                                double *deviation, double *smoothed, double *distance, int *tri_index,
                                unsigned char *region, unsigned char *status, double *target, unsigned char *owned,
                                size_t cap, ppp_mesh_deviation_tile_stats *part);
int ppp_get_mesh_signed_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp,
                                       double *signed_distance, double *smoothed, double *distance, int *tri_index,
                                       unsigned char *region, unsigned char *feature, unsigned char *flags,
                                       unsigned char *status, double *target, unsigned char *owned,
                                       size_t cap, ppp_mesh_signed_deviation_tile_stats *part);
int ppp_merge_mesh_deviation_tiles(size_t tiles, const ppp_mesh_deviation_tile_stats *parts, const double *const *v,
                                   const unsigned char *const *status, const double *const *target,
                                   const unsigned char *const *owned, ppp_mesh_deviation_stats *stats);
int ppp_merge_mesh_signed_deviation_tiles(size_t tiles, const ppp_mesh_signed_deviation_tile_stats *parts,
                                          const double *const *v, const unsigned char *const *status,
                                          const double *const *target, const unsigned char *const *owned,
                                          ppp_mesh_signed_deviation_stats *stats);
int ppp_get_mesh_registration_terms_tile(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp,
                                         const double *T12, ppp_registration_row *row, ppp_registration_part *part);
int ppp_register_mesh_tiles(const ppp_handle *hs, const ppp_trimesh *ms, size_t count,
                            const ppp_registration_params *rp, const double *T0_12, ppp_registration_row *rows,
                            size_t row_cap, ppp_register_tiles_stats *stats);
/* Spline::point(y) of slice s (include/Spline.h:22-25): xyz[3*i..] */
int ppp_eval_spline(ppp_handle h, int s, const double *y, size_t k, double *xyz);

/* ---- class Spline on caller-supplied knots (include/Spline.h:7-51) ----
 * The planner's own splines live with their slice (ppp_get_nodes / ppp_eval_spline above); these entry points serve callers
 * that construct a Spline themselves, as the reference's OnePath (path_slicing_alg.cpp:240-267), path_track
 * (Path_Generation.cpp:659-687) and dynamic_adjust_path (path_dynamic_alg.cpp:297-303, Spline::restart) do.
 * Knots and evaluation are double, as in GSL; the object owns its device copy of the knots and a HIP stream. */
typedef struct ppp_spline_s *ppp_spline;
/* Spline(int number, const double* point_y, const double* point_x, const double* point_z) (Spline.h:10-20): two
 * gsl_interp_steffen splines y -> x and y -> z.  Where GSL raises GSL_EINVAL and aborts -- fewer than 3 knots
 * (gsl_spline_alloc, steffen min_size 3) or y not strictly increasing (gsl_interp_init) -- PPP_ERR_ARG comes back. */
int ppp_spline_create(int device_id, size_t n, const double *y, const double *x, const double *z, ppp_spline *out);
/* Spline::restart (Spline.h:30-42): re-fit the same object on new knots */
int ppp_spline_restart(ppp_spline sp, size_t n, const double *y, const double *x, const double *z);
/* Spline::point(y) for k values (Spline.h:22-25): xyz[3*i..] = (splineYX(y), y, splineYZ(y)); a y outside [miny, bigy]
 * gives NaNs and PPP_ERR_DOMAIN (GSL_EDOM; GSL's default handler aborts there) */
int ppp_spline_eval(ppp_spline sp, const double *y, size_t k, double *xyz);
/* miny() / bigy() (Spline.h:27-28) and the knot count */
int ppp_spline_range(ppp_spline sp, double *miny, double *bigy, size_t *n);
int ppp_spline_destroy(ppp_spline sp);

/* ---- single-call mirrors of the reference's public methods ---- */
/* rangedX_index(int position) (path_slicing_alg.cpp:152-162, Path_Generation.cpp:94-104) */
int ppp_ranged_x_index(ppp_handle h, int position, int *out, size_t cap, size_t *n);
/* insert_point(indices, PlanePoint) (path_slicing_alg.cpp:164-237 / Path_Generation.cpp:107-206);
 * returns the MAP flattened in key order */
int ppp_insert_point(ppp_handle h, const int *indices, size_t n, float plane_x,
                     double *y, double *x, double *z, size_t cap, size_t *m);
/* estimate_normal() (path_slicing_alg.cpp:141-150) evaluated at the given cloud indices:
 * out4 = nx ny nz curvature */
int ppp_normals_at(ppp_handle h, const int *idx, size_t k, float *out4);
/* estimate_normal() over the WHOLE cloud (path_slicing_alg.cpp:141-150, Path_Generation.cpp:323-333):
 * out4 = n x 4 floats (nx ny nz curvature) in cloud index order; NaN where PCL gives NaN
 * (< 3 neighbours, dropped points).  SURVEY.md 8f rank 2. */
int ppp_estimate_normals(ppp_handle h, float *out4);
/* Area2Cloud(point, flag, key) of the dynamic adjustment (path_dynamic_alg.cpp:110-180) for k points
 * (xyz doubles, mm): key 0 = left boundary point (min x of the contact ellipse), 1 = right (max x);
 * out3 = k x 3 floats (NaN where the reference gets NaN) */
int ppp_area2cloud(ppp_handle h, const double *pts_xyz, size_t k, int key, float *out3);
/* compute_transform(point, principle_curvature) (path_dynamic_alg.cpp:77-107; v1 Path_Generation.cpp:362-400) for k query
 * points: out5 = k x (pcx pcy pcz pc1 pc2) -- the principal direction and the two curvatures computePointPrincipalCurvatures
 * returns for the curvature_k nearest neighbours of q, with the normal of the nearest one. NaN x 5 where q is not finite. */
int ppp_principal_curvatures_at(ppp_handle h, const float *q_xyz, size_t k, float *out5);
/* kdtree.nearestKSearch(q, 1) on the whole cloud for k query points */
int ppp_nearest(ppp_handle h, const float *q_xyz, size_t k, int *idx);

/* ---- intermediate stages of getPath, for stage-by-stage parity tests ---- */
enum { PPP_STAGE_WP_XYZ = 0,      /* W x 3 float: sampled points, mm (path_translation_alg.cpp:156-169) */
       PPP_STAGE_WP_NN = 1,       /* W int: nearest cloud index (:189)                                  */
       PPP_STAGE_WP_NORMAL = 2,   /* W x 4 float: normal + curvature (:190)                             */
       PPP_STAGE_WP_PRESMOOTH = 3,/* W x 6 float: after HandEyeTransform (:208)                         */
       PPP_STAGE_WP_SMOOTHED = 4  /* W x 6 float: after postion_smooth (:212)                           */ };
int ppp_get_stage(ppp_handle h, int stage, void *out, size_t cap_bytes, size_t *count);
/* sweeps of postion_smooth: always 0 -- the engine solves the sweeps' fixed point directly (one launch) */
int ppp_smooth_sweeps(ppp_handle h, int *sweeps);

/* ---- host-side file formats of the reference (no device work) ---- */
/* pcl::io::loadPCDFile<PointXYZRGB> (path_slicing_alg.cpp:10, Path_Generation.cpp:8): PCD v0.7,
 * DATA ascii | binary | binary_compressed (LZF, field-major), fields matched by name, x y z as F4 or F8.
 * *xyz receives n x 3 packed floats allocated by the library (release with ppp_free); viewpoint = the 7
 * VIEWPOINT numbers (tx ty tz qw qx qy qz). */
int ppp_load_pcd(const char *path, float **xyz, size_t *n, float viewpoint[7]);
/* the header alone: how the file stores its points (what ppp_set_cloud_pcd decides on) */
typedef struct ppp_pcd_layout {
    int data_kind;                    /* 0 = ascii, 1 = binary, 2 = binary_compressed */
    size_t points;                    /* POINTS (or WIDTH x HEIGHT) */
    size_t record_bytes;              /* bytes of one point's record: the sum of SIZE x COUNT over FIELDS */
    int x_offset, y_offset, z_offset; /* where x, y, z sit in it */
    int xyz_float32;                  /* 1 when all three are F 4 */
    long long data_offset;            /* the byte after the DATA line */
    float viewpoint[7];
} ppp_pcd_layout;
int ppp_pcd_probe(const char *path, ppp_pcd_layout *layout);
/* binary: 0 = ascii (pcl::io::savePCDFileASCII, path_slicing_alg.cpp:138), 1 = binary, 2 = binary_compressed */
int ppp_save_pcd(const char *path, const float *xyz, size_t n, size_t stride_floats, const float viewpoint[7], int binary);
/* a pcl::PointXYZRGB cloud (FIELDS x y z rgb, colour packed 0x00RRGGBB): what show() would hand to the viewer
 * (path_slicing_alg.cpp:69-80); xyz = n x 3 packed floats, rgb = n x 3 bytes; binary: 0 = ascii, 1 = binary */
int ppp_save_pcd_rgb(const char *path, const float *xyz, const unsigned char *rgb, size_t n, const float viewpoint[7], int binary);
/* STL, the triangle soup of a CAD export.  A file is binary when its size is 84 + 50 x the uint32 count at byte 80 (tested before
 * the word `solid`: binary files may start with it): an 80-byte header, the count, 50-byte records (normal, three vertices,
 * attribute word) -- the stored normal is ignored.  Anything else is read as ASCII: `facet` ... `vertex x y z` tokens, case and
 * white space as loosely as the ASCII PCD reader takes them, numbers correctly rounded to float.  *verts9 receives n_tris x 9
 * floats (a.x a.y a.z b.x ... c.z) allocated by the library (ppp_free).  PPP_ERR_IO: truncated or malformed.
 * ppp_save_stl: binary 1 = binary, 0 = ASCII (%.9g: reads back to the same floats); the normal written is n / A2 in double
 * (n = (b - a) x (c - a), A2 its length), or zeros for a degenerate triangle. */
int ppp_load_stl(const char *path, float **verts9, size_t *n_tris);
int ppp_save_stl(const char *path, const float *verts9, size_t n_tris, int binary);
void ppp_free(void *p);
/* SectPath::read_config / path_generater::read_config (path_slicing_alg.cpp:32-67,
 * path_dynamic_alg.cpp:34-75): same key set and parsing rules; absent keys keep config.txt's values */
typedef struct ppp_config {
    ppp_params params;
    char path_file[512];      /* pathFile */
    double depth, adjust_threshold, toolthickness;
    int smooth_cloud, remove_outlier, alignment, dynamic_adjustment; /* parsed, outside the hot path */
} ppp_config;
void ppp_default_config(ppp_config *c);
int ppp_read_config(const char *path, ppp_config *c);
/* pathFile writer (path_translation_alg.cpp:216-228): "x y z r p y " per line, ostream defaults */
int ppp_write_path_file(const char *path, const float *wp6, size_t W);

/* ---- a planner queue: workpieces in, lists out, a few handles behind it taking turns ----
 * A pass is three dependent launches that leave most of the chip idle most of the time; passes enqueued on different handles (HIP
 * streams) overlap.  The queue keeps `lanes` handles (0 = 2: best for a stream of new clouds, 50 us per 1 M-point cloud against 88 on one
 * lane and 62 on three; replays of resident clouds do best on three handles, four and more collide on the runtime's hardware queues)
 * with the given parameters and gives workpiece k to lane k mod lanes: ppp_queue_submit waits for that lane's earlier pass,
 * takes the cloud -- already in device memory, untouched until ppp_queue_wait of this ticket has returned -- without waiting for
 * its bounds where the lane's plan allows (ppp_set_cloud_device_async) and enqueues its pass; ppp_queue_wait returns the finished
 * list (device pointer into the lane, W rows of 6 floats; valid until `lanes` more workpieces have been submitted) or the error the
 * workpiece ended with.  Everything a caller could do with the handles itself (ppp_queue_lane gives them out, e.g. for
 * ppp_get_waypoints of the lane that holds a ticket); not thread-safe: one submitting thread. */
typedef struct ppp_queue_s *ppp_queue;
int ppp_queue_create(int device, int lanes, const ppp_params *params, ppp_queue *q);
void ppp_queue_destroy(ppp_queue q);
int ppp_queue_submit(ppp_queue q, const float *xyz_dev, size_t n, size_t stride_bytes, const float *viewpoint, long long *ticket);
int ppp_queue_wait(ppp_queue q, long long ticket, size_t *W, const float **list_dev);
int ppp_queue_lanes(ppp_queue q);
ppp_handle ppp_queue_lane(ppp_queue q, int i);
const char *ppp_queue_last_error(ppp_queue q);

/* ---- which launch sequence plans a cloud ---- */
/* Plan reuse (default on).  The first cloud of a handle sizes the window path's LDS capacities from a census of its own windows
 * (one more launch behind the conversion pass of ppp_set_cloud*).  A later cloud with the same point count and parameters, whose
 * slice walk has the same length and pad, inherits those capacities (+4 %) and skips that launch -- a planner that is fed one scan
 * after the other (the constructors of the reference's planner classes: src/Path_Alg/path_slicing_alg.cpp:3-30) saves it on every
 * workpiece.  The pass checks every window against its capacity on the device; one that does not fit makes the engine plan this
 * cloud again from its own census and repeat the pass (same results, one wasted pass).
 * Such a later cloud need not be waited for either: while the handle holds that window plan, ppp_set_cloud_device_async and
 * ppp_set_cloud_pcd (the calls whose points no caller takes back at once) only enqueue the conversion pass and return, and ppp_run_async / ppp_gen_path_async / ppp_get_path_async put the new cloud's pass behind it on
 * the earlier plan; bounds, walk and capacities are checked on the device against the record the conversion pass leaves, and any
 * other call (ppp_sync included) first reads that record and plans the cloud as a waiting ppp_set_cloud* would have -- a pass the
 * plan did not fit is repeated by the engine.  An error of the new cloud itself (no finite point, ...) then surfaces at that
 * call instead of at the call that set the cloud.  0 turns both off (PPP_NO_DEFERRED_PLAN=1 in the environment: the waiting only). */
int ppp_set_plan_reuse(ppp_handle h, int on);
/* How many handles the caller runs side by side on this device (default 1).  From two on the plan trades a little of a pass's own
 * latency for room on the CUs: the per-slice workgroups of small windows stay at 512 threads, so that a neighbouring pass's binning
 * and finish workgroups fit beside them; from three on the binning launch of a large cloud narrows too (ppp_get_binning_form) (1 M points / 256 slices on three handles: 0.038 -> 0.029 ms per workpiece; one pass alone
 * 0.065 -> 0.068 ms).  Same lists either way.  ppp_queue_create sets it on its lanes. */
int ppp_set_side_by_side(ppp_handle h, int handles);
/* The form of the window path's binning launch in THIS HANDLE'S plan: threads of a workgroup and points per thread (both 0 while
 * the plan runs the slab-index path).  1024 threads for a pass alone; 512 threads x 16 points where ppp_set_side_by_side announced
 * three or more handles and the cloud is large (about 0.8 M points and more; measured on 1 M points / 256 slices: two handles lose
 * with it and keep the form of a pass alone, four neither gain nor lose).  It is the form of the handle's own launches
 * (ppp_run_async, ppp_gen_path_async).  A batch (ppp_run_batch_async) launches once for all members: in this form only if every
 * member planned this same form, none bins through the staged form and the batch's slices together are no launch of several rounds
 * of workgroups; otherwise in the 1024-thread form.  The getter does not report a batch's launch. */
int ppp_get_binning_form(ppp_handle h, int *threads, int *points_per_thread);
/* The wave priorities (0..3, the hardware's; 0 is what a wave starts with) that THIS HANDLE'S plan launches the window pass with: the
 * binning, the per-slice and the finish launch.  All 0 for a pass alone and on the slab-index path.  Where ppp_set_side_by_side
 * announced two or more handles and the windows are small (the condition of the 512-thread slice workgroups), the finish launch --
 * the last link of a pass's chain of three dependent launches, the one the handle's next pass waits for -- runs above the waves
 * of the passes next door; the other two stay at 0 (raising the per-slice launch was measured to change nothing).  Priorities
 * order instruction issue only: the lists are the same bit for bit.  As ppp_get_binning_form, the getter reports the handle's own
 * launches, not a batch's. */
int ppp_get_launch_priorities(ppp_handle h, int *binning, int *per_slice, int *finish);
/* The engine has two launch sequences for the same hot path, with the same results up to the last bits of the normals'
 * float sums (both within the tolerances of tests/): the WINDOW path (three launches: every point binned once into the
 * window of its slice, one fused per-slice kernel, the finish; kd pairing, no dynamic adjustment / alignment, tool steps
 * wide enough that the slices' +-pad windows do not overlap, windows that fit a workgroup's LDS) and the SLAB-INDEX path
 * (six launches, any parameters; also what the single-call mirrors and the dynamic adjustment search).  The plan picks the
 * window path whenever it applies; a pass whose windows overflow or whose searches reach beyond them is repeated on the
 * slab-index path by itself.  ppp_set_fast_path(h, 0) keeps a handle on the slab-index path (tests, comparisons);
 * ppp_get_fast_path tells which one the current plan uses. */
int ppp_set_fast_path(ppp_handle h, int on);
int ppp_get_fast_path(ppp_handle h, int *active);

/* ---- measurement ---- */
/* When enabled every kernel launch is bracketed by hipEvents on the handle's stream. */
int ppp_enable_timing(ppp_handle h, int on);
/* names: cap entries of 48 chars; ms: time of each kernel since the last call, summed over its
 * launches; launches (may be NULL): how many launches that sum covers */
int ppp_get_kernel_times(ppp_handle h, char *names, float *ms, int *launches, size_t cap, size_t *n);

#ifdef __cplusplus
}
#endif
#endif
