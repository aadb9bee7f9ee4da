/*
 * ppp_mesh.h -- a triangle mesh sampled into a resident cloud (ppp_set_cloud_mesh): the nominal part as a CAD
 * export gives it.  Deterministic: the same mesh, pitch and facing give the same samples, bit for bit, in the same order.
 *
 * The rule, on the resident vertices (what ppp_set_cloud's conversion makes of the file's floats) widened to double, with one
 * rounding per written operation (+ - * /, sqrt, ceil; the unit is built with -ffp-contract=off).  Triangle f = (a, b, c):
 *   squared edge lengths ab, bc, ca, each (dx dx + dy dy) + dz dz; the vertices are rotated cyclically so that the longest edge is
 *   (p0, p1) and p2 lies opposite (ties: the first of ab, bc, ca); e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2,
 *   A2 = sqrt((nx nx + ny ny) + nz nz), L = sqrt(longest), hgt = A2 / L;
 *   degenerate (skipped): an index outside [0, n_verts), a coordinate that is not finite, A2 zero or not finite;
 *   culled (PPP_MESH_FRONT, skipped): unless ((nx (vx - p0x) + ny (vy - p0y)) + nz (vz - p0z)) > 0;
 *   rows R = max(1, ceil(hgt / pitch)); row r: t = (r + 0.5) / R, len = L (1 - t), M_r = max(1, ceil(len / pitch));
 *   column k of row r: s = (k + 0.5) / M_r, w = s (1 - t), sample = (p0 + e2 t) + e1 w per coordinate, rounded to float.
 * Rows run parallel to the longest edge, so their count follows the triangle's height: a sliver is one row, not one row per
 * pitch of its length.  Samples are ordered by triangle, row, column.
 *
 * Three kernels with two device-wide exclusive scans between them (ppp_scan_exclusive_u32, ppp_sort.h): one thread per triangle
 * writes its row count, one thread per row its column count, one thread per sample its point; a thread finds its row and its
 * triangle by upper-bound searches of the offsets and recomputes what it needs.  No thread loops over a triangle's rows or
 * samples: one large facet is as parallel as many small ones.
 */
#pragma once
#include <hip/hip_runtime.h>

/* ppp_preproc.hip owns the sampler's kernels.  ppp_scan.hip includes this header for the triangle frame (mesh_triangle,
   mesh_owner) and defines PPP_MESH_KERNELS_FOREIGN: the kernels are templates there and, never launched, never instantiated
   (PPP_KERNEL's idiom, ppp_kernels.h). */
#ifdef PPP_MESH_KERNELS_FOREIGN
#define PPP_MESH_KERNEL template <typename PPP_NEVER_ = void> __global__
#else
#define PPP_MESH_KERNEL __global__
#endif

#define MESH_T 256
/* counts above this are written as this: the sums then saturate (ppp_scan_exclusive_u32) and the host refuses them */
#define MESH_COUNT_MAX 0x80000000u

struct MeshArgs {
    const float *Vx, *Vy, *Vz; /* resident vertices */
    int n_verts;
    const int *tris;           /* n_tris x 3 indices, or nullptr: a soup (triangle f = vertices 3f, 3f + 1, 3f + 2) */
    int n_tris;
    double pitch;
    int front;                 /* PPP_MESH_FRONT */
    double vp[3];
};

/* the last entry of off[0 .. n] (ascending, off[0] = 0, off[n] > v) that is <= v: where entries repeat (empty triangles) the last
   of them, which is the one that owns v */
__device__ inline int mesh_owner(const unsigned *__restrict__ off, int n, unsigned v)
{
    int lo = 0, hi = n; /* off[lo] <= v < off[hi] */
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline double mesh_len2(const double a[3], const double b[3])
{
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline unsigned mesh_count(double quotient)
{
    const double c = ceil(quotient);
    if (!(c > 1.0)) return 1u; /* max(1, .) */
    return c >= (double)MESH_COUNT_MAX ? MESH_COUNT_MAX : (unsigned)c;
}

/* the vertices of triangle f, rotated: p0, p1 span the longest edge.  false: an index out of range or a coordinate that is not
   finite.  *longest = that edge's squared length; *rot (where asked): the caller's corner that became p0. */
__device__ inline bool mesh_triangle(const MeshArgs &A, int f, double p0[3], double p1[3], double p2[3], double *longest, int *rot = nullptr)
{
    int id[3];
    if (A.tris) { id[0] = A.tris[3 * (size_t)f]; id[1] = A.tris[3 * (size_t)f + 1]; id[2] = A.tris[3 * (size_t)f + 2]; }
    else { id[0] = 3 * f; id[1] = 3 * f + 1; id[2] = 3 * f + 2; }
    double v[3][3];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const bool in = id[q] >= 0 && id[q] < A.n_verts;
        const int i = in ? id[q] : 0;
        v[q][0] = (double)A.Vx[i]; v[q][1] = (double)A.Vy[i]; v[q][2] = (double)A.Vz[i];
        ok = ok && in && isfinite(v[q][0]) && isfinite(v[q][1]) && isfinite(v[q][2]);
    }
    if (!ok) return false;
    const double ab = mesh_len2(v[0], v[1]), bc = mesh_len2(v[1], v[2]), ca = mesh_len2(v[2], v[0]);
    const int first = (ab >= bc && ab >= ca) ? 0 : (bc >= ca ? 1 : 2);
    *longest = first == 0 ? ab : (first == 1 ? bc : ca);
    if (rot) *rot = first;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        p0[d] = first == 0 ? v[0][d] : (first == 1 ? v[1][d] : v[2][d]);
        p1[d] = first == 0 ? v[1][d] : (first == 1 ? v[2][d] : v[0][d]);
        p2[d] = first == 0 ? v[2][d] : (first == 1 ? v[0][d] : v[1][d]);
    }
    return true;
}

/* one thread per triangle: R, or 0 for a triangle that is skipped (counted in cnt[0] degenerate, cnt[1] culled).  Thread
   n_tris writes the closing 0 whose scan is the total. */
PPP_MESH_KERNEL void __launch_bounds__(MESH_T) k_mesh_rows(MeshArgs A, unsigned *__restrict__ R, unsigned *cnt)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f > A.n_tris) return;
    if (f == A.n_tris) { R[f] = 0u; return; }
    double p0[3], p1[3], p2[3], longest = 0.0;
    unsigned rows = 0u;
    int skipped = 0; /* 1 degenerate, 2 culled */
    if (!mesh_triangle(A, f, p0, p1, p2, &longest)) skipped = 1;
    else {
        const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double A2 = sqrt((nx * nx + ny * ny) + nz * nz);
        if (!(A2 > 0.0) || !isfinite(A2)) skipped = 1;
        else if (A.front && !(((nx * (A.vp[0] - p0[0]) + ny * (A.vp[1] - p0[1])) + nz * (A.vp[2] - p0[2])) > 0.0)) skipped = 2;
        else {
            const double L = sqrt(longest), hgt = A2 / L;
            rows = mesh_count(hgt / A.pitch);
        }
    }
    R[f] = rows;
    if (skipped) atomicAdd(&cnt[skipped - 1], 1u);
}

/* one thread per row: M_r.  Thread `rows` writes the closing 0. */
PPP_MESH_KERNEL void __launch_bounds__(MESH_T) k_mesh_cols(MeshArgs A, const unsigned *__restrict__ row_off, unsigned rows, unsigned *__restrict__ M)
{
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > rows) return;
    if (g == rows) { M[g] = 0u; return; }
    const int f = mesh_owner(row_off, A.n_tris, g);
    const unsigned r = g - row_off[f], R = row_off[f + 1] - row_off[f];
    double p0[3], p1[3], p2[3], longest = 0.0;
    (void)mesh_triangle(A, f, p0, p1, p2, &longest); /* (a triangle with rows passed every test) */
    const double L = sqrt(longest);
    const double t = ((double)r + 0.5) / (double)R, len = L * (1.0 - t);
    M[g] = mesh_count(len / A.pitch);
}

/* one thread per sample: its row, its triangle, its point (xyz packed: consecutive threads write consecutive records) */
PPP_MESH_KERNEL void __launch_bounds__(MESH_T) k_mesh_fill(MeshArgs A, const unsigned *__restrict__ row_off, const unsigned *__restrict__ col_off,
                                                      unsigned rows, unsigned samples, float *__restrict__ xyz, int *__restrict__ tri_index)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= samples) return;
    const int g = mesh_owner(col_off, (int)rows, i);
    const unsigned k = i - col_off[g], M = col_off[g + 1] - col_off[g];
    const int f = mesh_owner(row_off, A.n_tris, (unsigned)g);
    const unsigned r = (unsigned)g - row_off[f], R = row_off[f + 1] - row_off[f];
    double p0[3], p1[3], p2[3], longest = 0.0;
    (void)mesh_triangle(A, f, p0, p1, p2, &longest);
    const double t = ((double)r + 0.5) / (double)R, s = ((double)k + 0.5) / (double)M, w = s * (1.0 - t);
    float *o = xyz + 3 * (size_t)i;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double e1 = p1[d] - p0[d], e2 = p2[d] - p0[d];
        o[d] = (float)((p0[d] + e2 * t) + e1 * w);
    }
    if (tri_index) tri_index[i] = f;
}
