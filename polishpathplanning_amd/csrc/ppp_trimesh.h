/*
 * ppp_trimesh.h -- a resident triangle mesh with a uniform grid over its triangles, and the exact point-to-triangle search
 * against it (ppp_trimesh_create, ppp_trimesh_nearest, ppp_get_mesh_deviation).  The rule is the comment of
 * include/ppp_hip.h: the triangle frame of the mesh sampler (mesh_triangle, ppp_mesh.h), Ericson's region walk in double with one
 * rounding per written operation, the minimum over (D2, f).  The grid only decides which triangles a query looks at: the answer
 * is the brute force's over all indexed triangles, bit for bit, whatever the cell.
 *
 * The build, in the sampler's style: one thread per triangle marks it indexed or degenerate and reduces the box (integer maxima
 * of ordered keys), a scan ranks the indexed ones, one thread per indexed triangle writes its 48-byte record; one thread per
 * record counts the cells its box overlaps, a scan offsets them, one thread per (triangle, cell) pair writes (cell key, record) --
 * it finds its record with mesh_owner --, the radix sort orders the pairs by key (stable: records, and with them the caller's
 * indices, ascend inside a cell), and a boundary kernel writes cell_start.  No thread loops over a triangle's cells.  No float
 * atomics.
 */
#pragma once
#include "ppp_mesh.h"
#include "ppp_deviation.h"

#define TM_T 256
#define TM_MAX_CELLS (1u << 24)
#define TM_MAX_PAIRS 0x7ffffffeu /* the pair list stays below 2^31 - 1 */
#define TM_SIDE_SCALE 4294967296.0 /* 2^32: a box side over the mesh's largest extent, in fixed point */

/* one record per indexed triangle, three 16-byte loads: the nine rotated resident floats, f, the index in the caller's list, and
   rot, the caller's corner that the rotation made p0 (the search does not read it: the topology does, ppp_trimesh_topology.h) */
struct TriRec { float4 a, b, c; }; /* a = (p0x p0y p0z p1x), b = (p1y p1z p2x p2y), c = (p2z, f as bits, rot as bits, 0) */
static_assert(sizeof(TriRec) == 48, "a record is 48 bytes");

/* the grid as the kernels see it: by value */
struct TriGrid {
    const TriRec *rec;            /* [indexed] */
    const unsigned *cell_start;   /* [cells + 1] into cell_rec */
    const int *cell_rec;          /* [pairs] record numbers, by cell, ascending inside a cell */
    int indexed;
    int dim[3];
    double mn[3], mx[3];          /* the box of the indexed triangles' vertices (floats, widened) */
    double cell;                  /* (a float, widened) */
    int by_viewpoint;             /* PPP_TRIMESH_VIEWPOINT */
    double vp[3];
};

/* The cell of coordinate x on one axis, clamped into [0, dim): floor((x - mn) / cell) in double.  Both roundings are monotone,
   so x <= y gives tm_cell(x) <= tm_cell(y): a triangle is listed in every cell from its box's lower corner's to its upper
   corner's, and the search reads a query's cell by the same expression.  The host sizes the grid with it too. */
__host__ __device__ inline int tm_cell(double x, double mn, double cell, int dim)
{
    const double c = floor((x - mn) / cell);
    if (!(c > 0.0)) return 0; /* (a NaN too) */
    return c >= (double)dim ? dim - 1 : (int)c;
}

__device__ inline void tm_load(const TriRec *__restrict__ rec, int r, double a[3], double b[3], double c[3], int *f)
{
    const float4 u = rec[r].a, v = rec[r].b, w = rec[r].c;
    a[0] = (double)u.x; a[1] = (double)u.y; a[2] = (double)u.z;
    b[0] = (double)u.w; b[1] = (double)v.x; b[2] = (double)v.y;
    c[0] = (double)v.z; c[1] = (double)v.w; c[2] = (double)w.x;
    *f = __float_as_int(w.y);
}

/* N = e1 x e2 of the rotated frame and A2 = |N|, the sampler's expressions */
__device__ inline double tm_normal(const double p0[3], const double p1[3], const double p2[3], double N[3])
{
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    N[0] = e1[1] * e2[2] - e1[2] * e2[1]; N[1] = e1[2] * e2[0] - e1[0] * e2[2]; N[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
}

/* one thread per triangle: valid[f] = 1 for an indexed triangle, 0 for a degenerate one (7s's set); thread n_tris writes the
   closing 0 whose scan is the count.  bb[0 .. 2]: the largest complement of a lower coordinate's key, bb[3 .. 5]: the largest
   key of an upper coordinate (ordered_key; 0 = none): integer maxima, a wave's first, then one atomic per wave and word. */
__global__ void __launch_bounds__(TM_T) k_tm_bounds(MeshArgs A, unsigned *__restrict__ valid, unsigned *bb)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned k[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (f < A.n_tris) {
        double p0[3], p1[3], p2[3], N[3], longest = 0.0;
        bool ok = mesh_triangle(A, f, p0, p1, p2, &longest);
        if (ok) {
            const double A2 = tm_normal(p0, p1, p2, N);
            ok = A2 > 0.0 && isfinite(A2);
        }
        valid[f] = ok ? 1u : 0u;
        if (ok) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double lo = fmin(p0[d], fmin(p1[d], p2[d])), hi = fmax(p0[d], fmax(p1[d], p2[d]));
                k[d] = ~ordered_key((float)lo); k[3 + d] = ordered_key((float)hi); /* (floats widened: the casts are exact) */
            }
        }
    } else if (f == A.n_tris) valid[f] = 0u;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const unsigned m = wave_max_bits(k[d]);
        if ((threadIdx.x & 63) == 0 && m) atomicMax(bb + d, m);
    }
}

/* one thread per triangle: an indexed one writes its record at its rank */
__global__ void __launch_bounds__(TM_T) k_tm_records(MeshArgs A, const unsigned *__restrict__ rank, TriRec *__restrict__ rec)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.n_tris || rank[f + 1] == rank[f]) return;
    double p0[3], p1[3], p2[3], longest = 0.0;
    int rot = 0;
    (void)mesh_triangle(A, f, p0, p1, p2, &longest, &rot); /* (an indexed triangle passed every test) */
    TriRec R;
    R.a = make_float4((float)p0[0], (float)p0[1], (float)p0[2], (float)p1[0]);
    R.b = make_float4((float)p1[1], (float)p1[2], (float)p2[0], (float)p2[1]);
    R.c = make_float4((float)p2[2], __int_as_float(f), __int_as_float(rot), 0.f);
    rec[rank[f]] = R;
}

/* the cells [lo, hi] per axis that the box of record r overlaps */
__device__ inline void tm_cell_range(const TriGrid &G, int r, int lo[3], int hi[3])
{
    double a[3], b[3], c[3];
    int f;
    tm_load(G.rec, r, a, b, c, &f);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = tm_cell(fmin(a[d], fmin(b[d], c[d])), G.mn[d], G.cell, G.dim[d]);
        hi[d] = tm_cell(fmax(a[d], fmax(b[d], c[d])), G.mn[d], G.cell, G.dim[d]);
    }
}

/* one thread per record: the longest side of its box over `extent` (the mesh's largest extent) in 2^-32, summed in a 64-bit
   integer -- a term is at most 2^32 and there are fewer than 2^28 of them --: the automatic cell's mean, the same in every run */
__global__ void __launch_bounds__(TM_T) k_tm_sides(TriGrid G, double extent, unsigned long long *sum)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long t = 0;
    if (r < G.indexed) {
        double a[3], b[3], c[3], side = 0.0;
        int f;
        tm_load(G.rec, r, a, b, c, &f);
#pragma unroll
        for (int d = 0; d < 3; ++d) side = fmax(side, fmax(a[d], fmax(b[d], c[d])) - fmin(a[d], fmin(b[d], c[d])));
        t = (unsigned long long)llrint(side / extent * TM_SIDE_SCALE);
    }
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(sum, t);
}

/* one thread per record: the number of cells its box overlaps, saturating (MESH_COUNT_MAX); thread `indexed` writes the closing 0 */
__global__ void __launch_bounds__(TM_T) k_tm_count(TriGrid G, unsigned *__restrict__ cnt)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > G.indexed) return;
    if (r == G.indexed) { cnt[r] = 0u; return; }
    int lo[3], hi[3];
    tm_cell_range(G, r, lo, hi);
    const unsigned long long c = (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) * (unsigned long long)(hi[2] - lo[2] + 1);
    cnt[r] = c >= MESH_COUNT_MAX ? MESH_COUNT_MAX : (unsigned)c; /* (at most 2^24 cells: never reached) */
}

/* one thread per (record, cell) pair: its record by mesh_owner, its cell by its number inside the record's block of cells, x fastest */
__global__ void __launch_bounds__(TM_T) k_tm_pairs(TriGrid G, const unsigned *__restrict__ off, unsigned pairs, unsigned *__restrict__ key, int *__restrict__ val)
{
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= pairs) return;
    const int r = mesh_owner(off, G.indexed, g);
    unsigned k = g - off[r];
    int lo[3], hi[3];
    tm_cell_range(G, r, lo, hi);
    const unsigned nx = (unsigned)(hi[0] - lo[0] + 1), ny = (unsigned)(hi[1] - lo[1] + 1);
    const int ix = lo[0] + (int)(k % nx); k /= nx;
    const int iy = lo[1] + (int)(k % ny), iz = lo[2] + (int)(k / ny);
    key[g] = ((unsigned)iz * (unsigned)G.dim[1] + (unsigned)iy) * (unsigned)G.dim[0] + (unsigned)ix;
    val[g] = r;
}

/* the boundaries: one thread per cell, and one behind the last: cell_start[c] = the first sorted pair whose key is >= c (a lower
   bound search: an empty cell gets the start of the next listed one, cell_start[cells] = pairs) */
__global__ void __launch_bounds__(TM_T) k_tm_cell_start(const unsigned *__restrict__ key, unsigned pairs, unsigned cells, unsigned *__restrict__ cell_start)
{
    const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > cells) return;
    unsigned lo = 0u, hi = pairs; /* key[i] < c for i < lo, key[i] >= c for i >= hi */
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (key[mid] < c) lo = mid + 1u; else hi = mid;
    }
    cell_start[c] = lo;
}

/* the longest run of one cell, for the statistics: one thread per cell, integer maximum */
__global__ void __launch_bounds__(TM_T) k_tm_max_per_cell(const unsigned *__restrict__ cell_start, unsigned cells, unsigned *mx)
{
    const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned v = c < cells ? cell_start[c + 1] - cell_start[c] : 0u;
    v = wave_max_bits(v);
    if ((threadIdx.x & 63) == 0 && v) atomicMax(mx, v);
}

/* The closest point of triangle (a, b, c) to p: Ericson's region walk as include/ppp_hip.h writes it out.  x: the point,
   returns the region (0 face, 1 edge, 2 vertex); *D2 = |p - x|^2. */
__device__ __attribute__((always_inline)) inline int tm_closest(const double p[3], const double a[3], const double b[3], const double c[3], double x[3], double *D2)
{
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    auto dot = [](const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; };
    int region;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    double d3 = 0.0, d4 = 0.0, d5 = 0.0, d6 = 0.0, vc = 0.0, vb = 0.0, va = 0.0;
    bool done = false;
    if (d1 <= 0.0 && d2 <= 0.0) { x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; region = 2; done = true; }
    if (!done) {
        const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
        d3 = dot(ab, bp); d4 = dot(ac, bp);
        if (d3 >= 0.0 && d4 <= d3) { x[0] = b[0]; x[1] = b[1]; x[2] = b[2]; region = 2; done = true; }
    }
    if (!done) {
        vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double v = d1 / (d1 - d3);
            x[0] = a[0] + ab[0] * v; x[1] = a[1] + ab[1] * v; x[2] = a[2] + ab[2] * v; region = 1; done = true;
        }
    }
    if (!done) {
        const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
        d5 = dot(ab, cp); d6 = dot(ac, cp);
        if (d6 >= 0.0 && d5 <= d6) { x[0] = c[0]; x[1] = c[1]; x[2] = c[2]; region = 2; done = true; }
    }
    if (!done) {
        vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
            x[0] = a[0] + ac[0] * w; x[1] = a[1] + ac[1] * w; x[2] = a[2] + ac[2] * w; region = 1; done = true;
        }
    }
    if (!done) {
        va = d3 * d6 - d5 * d4;
        if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
            const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
            x[0] = b[0] + (c[0] - b[0]) * w; x[1] = b[1] + (c[1] - b[1]) * w; x[2] = b[2] + (c[2] - b[2]) * w; region = 1;
        } else {
            const double den = 1.0 / ((va + vb) + vc), v = vb * den, w = vc * den;
            x[0] = (a[0] + ab[0] * v) + ac[0] * w; x[1] = (a[1] + ab[1] * v) + ac[1] * w; x[2] = (a[2] + ab[2] * v) + ac[2] * w; region = 0;
        }
    }
    const double ex = p[0] - x[0], ey = p[1] - x[1], ez = p[2] - x[2];
    *D2 = (ex * ex + ey * ey) + ez * ez;
    return region;
}

/* what a query's thread keeps: the smallest (D2, f), its record's closest point and region */
struct TmBest {
    double D2, x[3];
    int f, r, region;
};

__device__ __attribute__((always_inline)) inline void tm_visit_cell(const TriGrid &G, unsigned cell, const double p[3], TmBest &B)
{
    const unsigned s0 = G.cell_start[cell], s1 = G.cell_start[cell + 1];
    for (unsigned k = s0; k < s1; ++k) {
        const int r = G.cell_rec[k];
        double a[3], b[3], c[3], x[3], D2;
        int f;
        tm_load(G.rec, r, a, b, c, &f);
        const int region = tm_closest(p, a, b, c, x, &D2);
        if (D2 < B.D2 || (D2 == B.D2 && f < B.f)) { B.D2 = D2; B.f = f; B.r = r; B.region = region; B.x[0] = x[0]; B.x[1] = x[1]; B.x[2] = x[2]; }
    }
}

/* The stop bound's slack.  A triangle the walk has not seen misses the visited block on some axis d beyond a block face that is
   interior to the grid, so every point of it has a coordinate beyond that face (tm_cell is monotone) and inside the mesh's box;
   its distance to the query is at least the gap to that face on d, joined with the query's distances to the box on the other
   two axes.  The face and the gap are computed, and tm_cell rounds twice, so the gap gives way by TM_ABS times the magnitudes
   that enter it, and the squared bound by TM_REL of itself for the walk's own roundings in D2: both are many orders above
   double's 2^-53 and far below any cell. */
#define TM_ABS 9.094947017729282e-13 /* 2^-40 */
#define TM_REL 9.5367431640625e-07   /* 2^-20 */

/* The nearest indexed triangle of the grid to the finite query p by (D2, f): shells of cells around the query's (clamped) cell,
   until the best D2 lies strictly inside the bound, the bound is beyond md2, or the block covers the grid. */
__device__ inline void tm_nearest(const TriGrid &G, const double p[3], double md2, TmBest &B)
{
    B.D2 = INFINITY; B.f = 0x7fffffff; B.r = -1; B.region = 255; B.x[0] = B.x[1] = B.x[2] = 0.0;
    int c[3];
    double out[3]; /* the query's distance to the box per axis: every triangle lies inside the box */
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        c[d] = tm_cell(p[d], G.mn[d], G.cell, G.dim[d]);
        out[d] = p[d] < G.mn[d] ? G.mn[d] - p[d] : (p[d] > G.mx[d] ? p[d] - G.mx[d] : 0.0);
        out[d] = fmax(0.0, out[d] - TM_ABS * (fabs(p[d]) + fabs(G.mn[d]) + fabs(G.mx[d])));
    }
    const double o2[3] = {out[0] * out[0], out[1] * out[1], out[2] * out[2]};
    const int rmax = max(max(max(c[0], G.dim[0] - 1 - c[0]), max(c[1], G.dim[1] - 1 - c[1])), max(c[2], G.dim[2] - 1 - c[2]));
    for (int r = 0; r <= rmax; ++r) {
        const int lx = max(c[0] - r, 0), hx = min(c[0] + r, G.dim[0] - 1);
        const int ly = max(c[1] - r, 0), hy = min(c[1] + r, G.dim[1] - 1);
        const int lz = max(c[2] - r, 0), hz = min(c[2] + r, G.dim[2] - 1);
        for (int iz = lz; iz <= hz; ++iz)
            for (int iy = ly; iy <= hy; ++iy) {
                const unsigned row = ((unsigned)iz * (unsigned)G.dim[1] + (unsigned)iy) * (unsigned)G.dim[0];
                const bool inner = iz > c[2] - r && iz < c[2] + r && iy > c[1] - r && iy < c[1] + r; /* the row crossed the last block */
                if (!inner) {
                    for (int ix = lx; ix <= hx; ++ix) tm_visit_cell(G, row + (unsigned)ix, p, B);
                } else {
                    if (c[0] - r >= 0) tm_visit_cell(G, row + (unsigned)(c[0] - r), p, B);
                    if (c[0] + r <= G.dim[0] - 1) tm_visit_cell(G, row + (unsigned)(c[0] + r), p, B);
                }
            }
        /* the bound behind shell r */
        const int lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
        double bound2 = INFINITY;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double rest = d == 0 ? o2[1] + o2[2] : (d == 1 ? o2[0] + o2[2] : o2[0] + o2[1]);
            if (lo[d] > 0) {
                const double face = G.mn[d] + (double)lo[d] * G.cell;
                const double gap = fmax(0.0, (p[d] - face) - TM_ABS * (fabs(p[d]) + fabs(G.mn[d]) + fabs(face)));
                bound2 = fmin(bound2, gap * gap + rest);
            }
            if (hi[d] < G.dim[d] - 1) {
                const double face = G.mn[d] + (double)(hi[d] + 1) * G.cell;
                const double gap = fmax(0.0, (face - p[d]) - TM_ABS * (fabs(p[d]) + fabs(G.mn[d]) + fabs(face)));
                bound2 = fmin(bound2, gap * gap + rest);
            }
        }
        if (bound2 == INFINITY) break; /* the block covers the grid */
        bound2 = bound2 * (1.0 - TM_REL);
        if (B.D2 < bound2 || bound2 > md2) break;
    }
}

/* The search kernel: one thread per query.  q4 != nullptr: the nq indexed points of a handle in its slab order (their cloud
   index rides in w; the maps hold DROPPED / -1 / 255 / NaN before the launch, and points outside the index keep that);
   otherwise xyz: nq packed points in the caller's order, a point that is not finite is DROPPED here.  Every output is optional
   but status.  fix, d2f: the fixed-point term and the float distance that ppp_get_deviation's tail reads. */
struct TmOut {
    double *distance, *closest, *deviation;
    long long *fix;
    float *d2f;
    int *tri_index;
    unsigned char *region, *status;
};

/* k_mesh_nearest's body for one query (qx, qy, qz) whose entries go to `id`: the whole-cloud kernel and the tile form
   (k_mesht_nearest, ppp_mesh_tile.h) call it, so a point's entries are the same bits from either (mesh_reg_search_body's way). */
__device__ __forceinline__ void mesh_nearest_body(float qx, float qy, float qz, int id, const TriGrid &G, double md2, const TmOut &O)
{
    const double p[3] = {(double)qx, (double)qy, (double)qz};
    int st = PPP_DEV_DROPPED;
    TmBest B;
    B.D2 = INFINITY; B.f = 0x7fffffff; B.r = -1; B.region = 255;
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
        tm_nearest(G, p, md2, B);
        st = (B.r >= 0 && B.D2 <= md2) ? PPP_DEV_MATCHED : PPP_DEV_TOO_FAR;
    }
    const bool hit = st == PPP_DEV_MATCHED;
    double dev = dev_nan();
    if (hit) {
        double a[3], b[3], c[3], N[3];
        int f;
        tm_load(G.rec, B.r, a, b, c, &f);
        const double A2 = tm_normal(a, b, c, N);
        double n[3] = {N[0] / A2, N[1] / A2, N[2] / A2};
        if (G.by_viewpoint && ((N[0] * (G.vp[0] - a[0]) + N[1] * (G.vp[1] - a[1])) + N[2] * (G.vp[2] - a[2])) < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        const double ex = p[0] - B.x[0], ey = p[1] - B.x[1], ez = p[2] - B.x[2];
        dev = ((ex * n[0]) + ey * n[1]) + ez * n[2];
    }
    O.status[id] = (unsigned char)st;
    if (O.tri_index) O.tri_index[id] = hit ? B.f : -1;
    if (O.region) O.region[id] = hit ? (unsigned char)B.region : (unsigned char)255;
    if (O.distance) O.distance[id] = hit ? sqrt(B.D2) : dev_nan();
    if (O.closest) {
        double *o = O.closest + 3 * (size_t)id;
        o[0] = hit ? B.x[0] : dev_nan(); o[1] = hit ? B.x[1] : dev_nan(); o[2] = hit ? B.x[2] : dev_nan();
    }
    if (O.deviation) O.deviation[id] = dev;
    if (hit && O.fix) O.fix[id] = llrint(dev * DEV_FIXED);
    if (hit && O.d2f) O.d2f[id] = (float)B.D2;
}

__global__ void __launch_bounds__(TM_T) k_mesh_nearest(const float4 *__restrict__ q4, const float *__restrict__ xyz, int nq, const TriGrid G, double md2, TmOut O)
{
    const int t = blockIdx.x * TM_T + threadIdx.x;
    if (t >= nq) return;
    float qx, qy, qz;
    int id = t;
    if (q4) { const float4 q = q4[t]; qx = q.x; qy = q.y; qz = q.z; id = idx_of(q); }
    else { qx = xyz[3 * (size_t)t]; qy = xyz[3 * (size_t)t + 1]; qz = xyz[3 * (size_t)t + 2]; }
    mesh_nearest_body(qx, qy, qz, id, G, md2, O);
}

/* what the maps hold where the search does not write: a thread per cloud index */
__global__ void __launch_bounds__(TM_T) k_tm_fill(int n, double *__restrict__ distance, int *__restrict__ tri_index, unsigned char *__restrict__ region,
                                                  unsigned char *__restrict__ status)
{
    for (int i = blockIdx.x * TM_T + threadIdx.x; i < n; i += gridDim.x * TM_T) {
        distance[i] = dev_nan(); tri_index[i] = -1; region[i] = 255; status[i] = PPP_DEV_DROPPED;
    }
}

/* the matched points by region and the largest distance's bits (doubles >= +0 order as their bits): acc[0 .. 2], acc[3] */
__global__ void __launch_bounds__(TM_T) k_tm_region_stats(int n, const unsigned char *__restrict__ status, const unsigned char *__restrict__ region,
                                                          const double *__restrict__ distance, unsigned long long *acc)
{
    unsigned long long cnt[3] = {0, 0, 0}, far = 0;
    for (int i = blockIdx.x * TM_T + threadIdx.x; i < n; i += gridDim.x * TM_T) {
        if (status[i] != PPP_DEV_MATCHED) continue;
        const int g = region[i];
        cnt[0] += g == 0; cnt[1] += g == 1; cnt[2] += g == 2;
        far = max(far, (unsigned long long)__double_as_longlong(distance[i]));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cnt[k] = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && cnt[k]) atomicAdd(acc + k, cnt[k]);
    }
    far = wave_max_bits(far);
    if ((threadIdx.x & 63) == 0 && far) atomicMax(acc + 3, far);
}
