/*
 * ppp_preproc.hip -- the preprocessing calls of the C ABI (include/ppp_hip.h) on the resident cloud: ppp_trans2center, ppp_transform_cloud,
 * ppp_remove_outlier, ppp_voxel_down, ppp_smooth_mls, and what they share (the opening, the adoption of the filtered cloud,
 * the sensor-frame copy of an aligned cloud); and ppp_set_cloud_mesh, which makes a resident cloud of a triangle mesh.  The unit
 * owns the kernels of ppp_preproc.h, ppp_align.h and ppp_mesh.h; of the handle and
 * the plan it sees what ppp_handle.h declares.  Compiled with the engine's flags.
 */
#ifndef PPP_SINGLE_TU /* (a diagnostic build includes this file into the engine's unit) */
#define PPP_KERNELS_FOREIGN /* ppp_kernels.h, ppp_dynamic.h, ppp_compact.h: types and device helpers only -- their kernels are the engine's */
#endif
#include "ppp_handle.h"
#include "ppp_preproc.h"
#include "ppp_align.h"
#include "ppp_sort.h"
#include "ppp_mesh.h"
#include <cstring>

extern "C" {

namespace {

/* path_translation_alg.cpp:171-174: the cloud carried back by invTransAlign, with its own slab index (same point
   indices).  The cloud is fixed between runs, so this happens once per cloud change, not per getPath. */
int rebuild_back(ppp_handle h)
{
    if (!h->back) {
        int rc = ppp_create(h->device, &h->back);
        if (rc) return fail(h, rc, "sensor-frame handle");
    }
    ppp_handle b = h->back;
    b->P = h->P;
    b->P.tool_radius = 1.0e6; b->P.dynamic_adjustment = 0; b->P.slice_begin = 0; b->P.slice_end = 0; /* one slice: this handle only ever serves its index */
    b->n = h->n;
    memcpy(b->vp, h->vp, sizeof(b->vp));
    HIPCHK(h, b->X.ensure(h->n)); HIPCHK(h, b->Y.ensure(h->n)); HIPCHK(h, b->Z.ensure(h->n));
    if (h->n) {
        Mat34 M;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) M.m[r][c] = h->invTA[r][c];
        LAUNCH(h, "k_transform_se3", k_transform_se3, (unsigned)((h->n + 255) / 256), 256, 0, h->X.p, h->Y.p, h->Z.p, (int)h->n, M, b->X.p, b->Y.p, b->Z.p);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    b->big_path = false;
    int rc = refresh_bounds_and_plan(b);
    if (rc == PPP_OK) rc = index_ready(b);
    if (rc == PPP_OK) { hipError_t e = hipStreamSynchronize(b->stream); if (e != hipSuccess) rc = PPP_ERR_HIP; }
    if (rc != PPP_OK) return fail(h, rc, std::string("sensor-frame index: ") + b->err);
    return PPP_OK;
}

/* the resident cloud was replaced or moved: bounds, plan, and the sensor-frame copy when the cloud is aligned */
int cloud_changed(ppp_handle h)
{
    int rc = refresh_bounds_and_plan(h);
    if (rc == PPP_OK && h->aligned) rc = rebuild_back(h);
    return rc;
}

/* the opening of the preprocessing calls: a whole-cloud handle with a cloud, settled on its device.  bad_arg: the
   caller's message for an invalid argument, reported between the two checks (ppp_remove_outlier's order) */
int preproc_begin(ppp_handle h, const char *bad_arg = nullptr)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    { int rcs = settle(h); if (rcs) return rcs; }
    if (!h->have_cloud) return fail(h, PPP_ERR_ARG, "no cloud set");
    if (bad_arg) return fail(h, PPP_ERR_ARG, bad_arg);
    if (h->ranged || h->part_given) return fail(h, PPP_ERR_ARG, "preprocess the cloud on a whole-cloud handle");
    return PPP_OK;
}

/* the filtered cloud of n points replaces the resident one (filter(*cloud)).  The callers free their scratch first: hipFree
   waits for the device, and behind this call it would wait for the launches of the new plan. */
int adopt_cloud(ppp_handle h, DevBuf<float> &X2, DevBuf<float> &Y2, DevBuf<float> &Z2, size_t n)
{
    h->X = std::move(X2); h->Y = std::move(Y2); h->Z = std::move(Z2);
    h->n = n;
    h->drop_graph();
    return cloud_changed(h);
}

} // namespace

int ppp_trans2center(ppp_handle h, float *trans_align16, float *centroid3, float *covariance9)
{
    int rc = preproc_begin(h);
    if (rc) return rc;
    if (h->aligned) return fail(h, PPP_ERR_ARG, "the cloud is aligned already (TransAlign would be overwritten): set the cloud again");
    const int n = (int)h->n;
    if (n == 0 || h->h_nvalid == 0) return fail(h, PPP_ERR_ARG, "no finite point to align");
    float hs[6] = {0, 0, 0, 0, 0, 0}, c[3] = {0, 0, 0};
    const int hcnt = h->h_nvalid; /* the finite points, counted with the bounds */
    const unsigned gb = (unsigned)((n + 255) / 256);
    { /* scratch, freed before the re-plan (adopt_cloud) */
        const size_t stride = ((size_t)n + 3) & ~(size_t)3;
        DevBuf<float> V, sums;
        hipError_t e = V.ensure(6 * stride);
        if (e == hipSuccess) e = sums.ensure(8);
        if (e != hipSuccess) return fail(h, PPP_ERR_HIP, std::string("trans2center buffers: ") + hipGetErrorString(e));
        /* pcl::compute3DCentroid: three running float sums, / float(count) */
        LAUNCH(h, "k_seq_prep_centroid", k_seq_prep_centroid, gb, 256, 0, h->X.p, h->Y.p, h->Z.p, n, stride, V.p);
        LAUNCH(h, "k_seq_sum", k_seq_sum, 3, 64 * SEQ_WAVES, 0, V.p, stride, n, sums.p);
        HIPCHK(h, hipMemcpyAsync(hs, sums.p, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (hcnt <= 0) return fail(h, PPP_ERR_ARG, "no finite point to align");
        for (int d = 0; d < 3; ++d) c[d] = hs[d] / static_cast<float>(hcnt);
        /* pcl::computeCovarianceMatrix: six running float sums of float products */
        LAUNCH(h, "k_seq_prep_cov", k_seq_prep_cov, gb, 256, 0, h->X.p, h->Y.p, h->Z.p, n, c[0], c[1], c[2], stride, V.p);
        LAUNCH(h, "k_seq_sum", k_seq_sum, 6, 64 * SEQ_WAVES, 0, V.p, stride, n, sums.p);
        HIPCHK(h, hipMemcpyAsync(hs, sums.p, 6 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    float cov[3][3];
    cov[1][1] = hs[0]; cov[1][2] = hs[1]; cov[2][2] = hs[2]; cov[0][0] = hs[3]; cov[0][1] = hs[4]; cov[0][2] = hs[5];
    cov[1][0] = cov[0][1]; cov[2][0] = cov[0][2]; cov[2][1] = cov[1][2];
    if (centroid3) memcpy(centroid3, c, sizeof(c));
    if (covariance9) for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) covariance9[3 * i + j] = cov[i][j];
    ppp_align::EigenSolver3f es;
    es.compute(cov);
    if (es.complex_pair || !es.converged)
        return fail(h, PPP_ERR_DOMAIN, "trans2center: the float Schur form of the covariance keeps a complex pair (two equal extents) or did not converge");
    ppp_align::trans_align(es, c, h->TA);
    ppp_align::inverse4(h->TA, h->invTA);
    if (trans_align16) for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) trans_align16[4 * i + j] = h->TA[i][j];
    /* pcl::transformPointCloud(*cloud, *cloud, TransAlign) */
    Mat34 M;
    for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 4; ++cc) M.m[r][cc] = h->TA[r][cc];
    LAUNCH(h, "k_transform_se3", k_transform_se3, gb, 256, 0, h->X.p, h->Y.p, h->Z.p, n, M, h->X.p, h->Y.p, h->Z.p);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->aligned = true;
    h->drop_graph();
    return cloud_changed(h);
}

/* T applied to the resident cloud (the result of ppp_register): pcl::transformPointCloud's arithmetic with the float of T, in
   place, then what ppp_trans2center does behind its own transform -- but the cloud is not "aligned": no TransAlign is kept */
int ppp_transform_cloud(ppp_handle h, const double *T12)
{
    int rc = preproc_begin(h);
    if (rc) return rc;
    if (h->aligned) return fail(h, PPP_ERR_ARG, "transform_cloud: the cloud is aligned (ppp_trans2center): its sensor-frame copy would not follow");
    Mat34 M = {{{1.f, 0.f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.f, 1.f, 0.f}}};
    if (T12)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                if (!std::isfinite(T12[4 * r + c])) return fail(h, PPP_ERR_ARG, "transform_cloud: the transform has an entry that is not finite");
                M.m[r][c] = (float)T12[4 * r + c];
            }
    const int n = (int)h->n;
    if (n) LAUNCH(h, "k_transform_se3", k_transform_se3, (unsigned)((n + 255) / 256), 256, 0, h->X.p, h->Y.p, h->Z.p, n, M, h->X.p, h->Y.p, h->Z.p);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->drop_graph();
    return cloud_changed(h);
}

int ppp_remove_outlier(ppp_handle h, int mean_k, double stddev_mul, size_t *n_kept, double *threshold)
{
    int rc = preproc_begin(h, (mean_k < 1 || mean_k > 63) ? "mean_k must be in [1, 63]" : nullptr);
    if (rc) return rc;
    rc = index_ready(h);
    if (rc) return rc;
    const int n = (int)h->n, ns = h->hmeta.n_sorted;
    if (ns < mean_k + 1) return fail(h, PPP_ERR_ARG, "fewer finite points than mean_k + 1 (PCL reads past its neighbour vectors here)");
    /* first radius of the k-NN gather: mean_k + 1 points of a sheet of the cloud's mean areal density, +25 % */
    const double area = ((double)h->h_mx[0] - h->h_mn[0]) * ((double)h->h_mx[1] - h->h_mn[1]);
    const double rho = (area > 0 && h->h_nvalid > 0) ? (double)h->h_nvalid / area : 1.0;
    const float r0 = (float)std::max(0.5, 1.25 * std::sqrt((double)(mean_k + 1) / (3.14159265358979 * rho)));
    const int nblocks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK, nparts = std::max(1, std::min(1024, (n + 255) / 256));
    DevBuf<float> X2, Y2, Z2;
    SorStats hst;
    { /* scratch, freed before the re-plan (adopt_cloud) */
        DevBuf<float> dist;
        DevBuf<double> part;
        DevBuf<int> bcnt;
        DevBuf<SorStats> st;
        hipError_t e = dist.ensure(n);
        if (e == hipSuccess) e = X2.ensure(n);
        if (e == hipSuccess) e = Y2.ensure(n);
        if (e == hipSuccess) e = Z2.ensure(n);
        if (e == hipSuccess) e = part.ensure(2 * (size_t)nparts);
        if (e == hipSuccess) e = bcnt.ensure(nblocks);
        if (e == hipSuccess) e = st.ensure(1);
        if (e != hipSuccess) return fail(h, PPP_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        HIPCHK(h, hipMemsetAsync(dist.p, 0, sizeof(float) * (size_t)n, h->stream)); /* non-finite points: distance 0 */
        LAUNCH(h, "k_sor_dist", k_sor_dist, (unsigned)((ns + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, h->meta.p, h->sorted4.p, h->slab_start.p,
               h->slab_xmin.p, h->slab_xmax.p, mean_k, r0, dist.p);
        LAUNCH(h, "k_sor_partial", k_sor_partial, nparts, 256, 0, dist.p, n, part.p);
        LAUNCH(h, "k_sor_threshold", k_sor_threshold, 1, 256, 0, h->meta.p, part.p, nparts, stddev_mul, st.p);
        SorSel sel{dist.p, st.p, h->X.p, h->Y.p, h->Z.p, X2.p, Y2.p, Z2.p};
        rc = compact(h, sel, n, bcnt.p, &st.p->n_kept);
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(&hst, st.p, sizeof(SorStats), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->pass.meta_will_arrive(MetaAt::on_demand());
    rc = fetch_meta(h);
    if (rc == PPP_OK) rc = map_dev_err(h);
    if (rc) return rc;
    if (n_kept) *n_kept = (size_t)hst.n_kept;
    if (threshold) *threshold = hst.threshold;
    return adopt_cloud(h, X2, Y2, Z2, (size_t)hst.n_kept);
}

int ppp_voxel_down(ppp_handle h, float lx, float ly, float lz, size_t *n_out, int *overflow)
{
    int rc = preproc_begin(h);
    if (rc) return rc;
    if (!(lx > 0.f) || !(ly > 0.f) || !(lz > 0.f) || !std::isfinite(lx) || !std::isfinite(ly) || !std::isfinite(lz))
        return fail(h, PPP_ERR_ARG, "leaf sizes must be positive and finite");
    if (overflow) *overflow = 0;
    if (n_out) *n_out = h->n;
    const int n = (int)h->n;
    if (n == 0) return PPP_OK;
    /* voxel_grid.hpp applyFilter: inverse_leaf_size_ = 1 / leaf_size_ (float), the index-overflow test on the float extents,
       min_b_ / max_b_ / div_b_ / divb_mul_ */
    const float inv[3] = {1.0f / lx, 1.0f / ly, 1.0f / lz};
    VoxGrid g;
    long long cells = 1, dxyz = 1;
    int div_b[3];
    if (h->h_nvalid > 0) {
        for (int d = 0; d < 3; ++d) {
            dxyz *= (long long)((h->h_mx[d] - h->h_mn[d]) * inv[d]) + 1;
            const int min_b = (int)std::floor(h->h_mn[d] * inv[d]), max_b = (int)std::floor(h->h_mx[d] * inv[d]);
            div_b[d] = max_b - min_b + 1;
            cells *= div_b[d];
            g.inv[d] = inv[d];
            g.min_b[d] = (float)min_b;
            if (dxyz > 0x7fffffffLL || cells > 0x7fffffffLL || dxyz <= 0 || cells <= 0) {
                /* "Leaf size is too small for the input dataset. Integer indices would overflow.": output = input */
                if (overflow) *overflow = 1;
                return PPP_OK;
            }
        }
        g.mul[0] = 1; g.mul[1] = div_b[0]; g.mul[2] = div_b[0] * div_b[1];
    } else {
        for (int d = 0; d < 3; ++d) { g.inv[d] = inv[d]; g.min_b[d] = 0.f; g.mul[d] = 0; }
    }
    g.none = (unsigned)cells;
    int end_bit = 1;
    while (end_bit < 32 && (cells >> end_bit)) ++end_bit;
    const int nblocks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
    DevBuf<float> X2, Y2, Z2;
    int n_vox = 0;
    { /* scratch, freed before the re-plan (adopt_cloud) */
        DevBuf<unsigned> key, key2;
        DevBuf<int> idx, idx2, bcnt;
        DevBuf<char> tmp;
        DevBuf<float4> pts;
        size_t tmp_bytes = 0;
        hipError_t e = ppp_sort_pairs_u32(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, end_bit, h->stream);
        if (e == hipSuccess) e = key.ensure(n);
        if (e == hipSuccess) e = key2.ensure(n);
        if (e == hipSuccess) e = idx.ensure(n);
        if (e == hipSuccess) e = idx2.ensure(n);
        if (e == hipSuccess) e = bcnt.ensure((size_t)nblocks + 1); /* block counts, then the total */
        if (e == hipSuccess) e = tmp.ensure(tmp_bytes);
        if (e == hipSuccess) e = pts.ensure(n);
        if (e == hipSuccess) e = X2.ensure(n);
        if (e == hipSuccess) e = Y2.ensure(n);
        if (e == hipSuccess) e = Z2.ensure(n);
        if (e != hipSuccess) return fail(h, PPP_ERR_HIP, std::string("voxel_down buffers: ") + hipGetErrorString(e));
        const unsigned gb = (unsigned)((n + 255) / 256);
        LAUNCH(h, "k_vox_key", k_vox_key, gb, 256, 0, h->X.p, h->Y.p, h->Z.p, n, g, key.p, idx.p);
        HIPCHK(h, ppp_sort_pairs_u32(tmp.p, &tmp_bytes, key.p, key2.p, idx.p, idx2.p, (size_t)n, end_bit, h->stream));
        LAUNCH(h, "k_vox_gather", k_vox_gather, gb, 256, 0, h->X.p, h->Y.p, h->Z.p, idx2.p, n, pts.p);
        VoxHeadSel sel{key2.p, pts.p, n, g.none, X2.p, Y2.p, Z2.p};
        rc = compact(h, sel, n, bcnt.p, bcnt.p + nblocks);
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(&n_vox, bcnt.p + nblocks, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (n_out) *n_out = (size_t)n_vox;
    return adopt_cloud(h, X2, Y2, Z2, (size_t)n_vox);
}

int ppp_smooth_mls(ppp_handle h, double search_radius, int order, size_t *n_out)
{
    int rc = preproc_begin(h);
    if (rc) return rc;
    if (!(search_radius > 0) || !std::isfinite(search_radius)) return fail(h, PPP_ERR_ARG, "search radius must be positive"); /* mls.hpp: "Invalid search radius" */
    if (order < 0 || order > 3) return fail(h, PPP_ERR_ARG, "polynomial order must be in [0, 3]");
    rc = index_ready(h);
    if (rc) return rc;
    const int n = (int)h->n, ns = h->hmeta.n_sorted;
    if (n_out) *n_out = h->n;
    if (n == 0) return PPP_OK;
    const int nblocks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
    DevBuf<float> X2, Y2, Z2;
    int n_kept = 0;
    { /* scratch, freed before the re-plan (adopt_cloud) */
        DevBuf<float4> rec;
        DevBuf<int> bcnt;
        hipError_t e = rec.ensure(n);
        if (e == hipSuccess) e = X2.ensure(n);
        if (e == hipSuccess) e = Y2.ensure(n);
        if (e == hipSuccess) e = Z2.ensure(n);
        if (e == hipSuccess) e = bcnt.ensure((size_t)nblocks + 1); /* block counts, then the total */
        if (e != hipSuccess) return fail(h, PPP_ERR_HIP, std::string("smooth buffers: ") + hipGetErrorString(e));
        HIPCHK(h, hipMemsetAsync(rec.p, 0, sizeof(float4) * (size_t)n, h->stream));
        const unsigned gb = (unsigned)((std::max(ns, 1) + 255) / 256);
        const float rf = (float)search_radius;
        const double sq = search_radius * search_radius;
        if (order == 3) LAUNCH(h, "k_mls<3>", k_mls<3>, gb, 256, 0, h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_xmin.p, h->slab_xmax.p, rf, sq, rec.p);
        else if (order == 2) LAUNCH(h, "k_mls<2>", k_mls<2>, gb, 256, 0, h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_xmin.p, h->slab_xmax.p, rf, sq, rec.p);
        else LAUNCH(h, "k_mls<1>", k_mls<1>, gb, 256, 0, h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_xmin.p, h->slab_xmax.p, rf, sq, rec.p);
        MlsKeptSel sel{rec.p, X2.p, Y2.p, Z2.p};
        rc = compact(h, sel, n, bcnt.p, bcnt.p + nblocks);
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(&n_kept, bcnt.p + nblocks, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->pass.meta_will_arrive(MetaAt::on_demand());
    rc = fetch_meta(h);
    if (rc == PPP_OK) rc = map_dev_err(h);
    if (rc) return rc;
    if (n_out) *n_out = (size_t)n_kept;
    return adopt_cloud(h, X2, Y2, Z2, (size_t)n_kept);
}

/* ---- a triangle mesh sampled into the resident cloud (ppp_mesh.h) ---- */
void ppp_default_mesh_params(ppp_mesh_params *mp)
{
    if (!mp) return;
    mp->pitch = 0.5f; mp->facing = PPP_MESH_ALL;
}

namespace {
constexpr size_t MESH_CLOUD_MAX = 0x7fffffffu / 8; /* the points of a resident cloud (set_cloud_common) */
} // namespace

int ppp_set_cloud_mesh(ppp_handle h, const float *verts, size_t n_verts, const int *tris, size_t n_tris, const ppp_mesh_params *mp,
                       const float *viewpoint, int *tri_index, size_t cap, ppp_mesh_stats *stats)
{
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!h) return PPP_ERR_ARG;
    if (!verts || !mp) return fail(h, PPP_ERR_ARG, "set_cloud_mesh: vertices and parameters are required");
    if (!(mp->pitch > 0.f) || !std::isfinite(mp->pitch)) return fail(h, PPP_ERR_ARG, "set_cloud_mesh: the pitch must be positive and finite");
    if (mp->facing != PPP_MESH_ALL && mp->facing != PPP_MESH_FRONT) return fail(h, PPP_ERR_ARG, "set_cloud_mesh: facing is PPP_MESH_ALL or PPP_MESH_FRONT");
    if (n_tris == 0) return fail(h, PPP_ERR_ARG, "set_cloud_mesh: no triangle");
    if (!tris && (n_verts % 3 || n_verts / 3 != n_tris)) return fail(h, PPP_ERR_ARG, "set_cloud_mesh: a soup (tris == NULL) has three vertices per triangle");
    if (n_tris > MESH_CLOUD_MAX || n_verts > MESH_CLOUD_MAX) return fail(h, PPP_ERR_CAPACITY, "set_cloud_mesh: mesh too large");
    if (stats) stats->triangles = n_tris;
    HIPCHK(h, hipSetDevice(h->device));
    { int rcs = settle(h); if (rcs) return rcs; }
    if (h->part_given) return fail(h, PPP_ERR_UNSUPPORTED, "set_cloud_mesh: this handle holds a part (ppp_set_cloud_part): a mesh is sampled whole");
    size_t samples = 0;
    { /* scratch, freed before the plan of the new cloud */
        DevBuf<char> raw, tmp;
        DevBuf<float> V;
        DevBuf<int> T, tri_dev;
        DevBuf<unsigned> R, row_off, M, col_off, cnt;
        const size_t nv = std::max<size_t>(n_verts, 1);
        hipError_t e = raw.ensure(12 * nv);
        if (e == hipSuccess) e = V.ensure(3 * nv);
        if (e == hipSuccess && tris) e = T.ensure(3 * n_tris);
        if (e == hipSuccess) e = R.ensure(n_tris + 1);
        if (e == hipSuccess) e = row_off.ensure(n_tris + 1);
        if (e == hipSuccess) e = cnt.ensure(2);
        if (e != hipSuccess) return fail(h, PPP_ERR_HIP, std::string("set_cloud_mesh buffers: ") + hipGetErrorString(e));
        /* the vertices become resident ones by the conversion of every cloud (k_ingest) */
        if (n_verts) {
            HIPCHK(h, hipMemcpyAsync(raw.p, verts, 12 * n_verts, hipMemcpyHostToDevice, h->stream));
#ifdef PPP_KERNELS_FOREIGN /* (the engine's kernel, instantiated here: ppp_kernels.h) */
            LAUNCH(h, "k_ingest", k_ingest<>, (unsigned)((n_verts + 255) / 256), 256, 0, raw.p, (size_t)12, (int)n_verts, h->P.change_range, V.p, V.p + nv, V.p + 2 * nv);
#else
            LAUNCH(h, "k_ingest", k_ingest, (unsigned)((n_verts + 255) / 256), 256, 0, raw.p, (size_t)12, (int)n_verts, h->P.change_range, V.p, V.p + nv, V.p + 2 * nv);
#endif
        }
        if (tris) HIPCHK(h, hipMemcpyAsync(T.p, tris, 12 * n_tris, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(cnt.p, 0, 2 * sizeof(unsigned), h->stream));
        MeshArgs A;
        A.Vx = V.p; A.Vy = V.p + nv; A.Vz = V.p + 2 * nv; A.n_verts = (int)n_verts;
        A.tris = tris ? T.p : nullptr; A.n_tris = (int)n_tris;
        A.pitch = (double)mp->pitch; A.front = mp->facing == PPP_MESH_FRONT;
        for (int d = 0; d < 3; ++d) A.vp[d] = viewpoint ? (double)viewpoint[d] : 0.0;
        LAUNCH(h, "k_mesh_rows", k_mesh_rows, (unsigned)((n_tris + 1 + MESH_T - 1) / MESH_T), MESH_T, 0, A, R.p, cnt.p);
        { int rc = scan_exclusive(h, "mesh_scan_rows", tmp, R.p, row_off.p, n_tris + 1); if (rc) return rc; }
        unsigned hcnt[2] = {0, 0}, rows = 0;
        HIPCHK(h, hipMemcpyAsync(hcnt, cnt.p, sizeof(hcnt), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&rows, row_off.p + n_tris, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (stats) { stats->degenerate = hcnt[0]; stats->culled = hcnt[1]; stats->sampled = n_tris - hcnt[0] - hcnt[1]; stats->rows = rows; }
        if (rows == 0) return fail(h, PPP_ERR_ARG, "set_cloud_mesh: no sample: every triangle is degenerate or culled");
        if (rows > MESH_CLOUD_MAX) return fail(h, PPP_ERR_CAPACITY, "set_cloud_mesh: too many rows for a resident cloud: the pitch is too small for this mesh");
        e = M.ensure((size_t)rows + 1);
        if (e == hipSuccess) e = col_off.ensure((size_t)rows + 1);
        if (e != hipSuccess) return fail(h, PPP_ERR_HIP, std::string("set_cloud_mesh buffers: ") + hipGetErrorString(e));
        LAUNCH(h, "k_mesh_cols", k_mesh_cols, (unsigned)(((size_t)rows + 1 + MESH_T - 1) / MESH_T), MESH_T, 0, A, row_off.p, rows, M.p);
        { int rc = scan_exclusive(h, "mesh_scan_cols", tmp, M.p, col_off.p, (size_t)rows + 1); if (rc) return rc; }
        unsigned total = 0;
        HIPCHK(h, hipMemcpyAsync(&total, col_off.p + rows, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (stats) stats->samples = total;
        if (total > MESH_CLOUD_MAX) return fail(h, PPP_ERR_CAPACITY, "set_cloud_mesh: too many samples for a resident cloud: the pitch is too small for this mesh");
        samples = total;
        const size_t k = tri_index ? std::min(cap, samples) : 0;
        /* the samples land where the points of ppp_set_cloud do: the handle's staging buffer, as packed records */
        HIPCHK(h, h->scratch.ensure(12 * samples));
        if (k) HIPCHK(h, tri_dev.ensure(samples));
        LAUNCH(h, "k_mesh_fill", k_mesh_fill, (unsigned)((samples + MESH_T - 1) / MESH_T), MESH_T, 0, A, row_off.p, col_off.p, rows, total,
               (float *)h->scratch.p, k ? tri_dev.p : nullptr);
        if (k) HIPCHK(h, hipMemcpyAsync(tri_index, tri_dev.p, k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    /* ... and go the way those points go, their conversion without the x1000: plan, bounds, viewpoint, caches as ppp_set_cloud leaves them */
    return set_cloud_resident(h, (const float *)h->scratch.p, samples, viewpoint);
}

int ppp_set_cloud_stl(ppp_handle h, const char *path, const ppp_mesh_params *mp, const float *viewpoint, ppp_mesh_stats *stats)
{
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!h) return PPP_ERR_ARG;
    if (!path) return fail(h, PPP_ERR_ARG, "set_cloud_stl: no file name");
    float *v9 = nullptr;
    size_t nt = 0;
    int rc = ppp_load_stl(path, &v9, &nt);
    if (rc != PPP_OK) return fail(h, rc, std::string("not a readable STL file: ") + path);
    rc = ppp_set_cloud_mesh(h, v9, 3 * nt, nullptr, nt, mp, viewpoint, nullptr, 0, stats);
    ppp_free(v9);
    return rc;
}

} // extern "C"
