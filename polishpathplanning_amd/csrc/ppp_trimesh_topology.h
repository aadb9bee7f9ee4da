/*
 * ppp_trimesh_topology.h -- the welded topology of a resident triangle mesh, its angle-weighted pseudonormals, and the sign of
 * the exact search's distance (ppp_trimesh_topology, ppp_trimesh_get_topology, ppp_trimesh_signed_nearest,
 * ppp_get_mesh_signed_deviation).  The rule is the comment of include/ppp_hip.h.
 *
 * Everything works on slots: slot j = 3 r + k is corner k, in the caller's corner order, of record r.  Records ascend with the
 * caller's triangle index f, so slots ascend with the corner index 3 f + k: "the smallest corner" is the smallest slot, and an
 * id is turned into 3 f + k only where it leaves the device (tt_corner_id).  Half-edge k of a record shares slot 3 r + k.
 *
 * The build: a thread per slot writes the three coordinate keys of its corner (-0 made +0); three stable radix passes (z, then
 * y, then x: ppp_sort_pairs_u32, the key of the next pass gathered through the order of the last) leave the corners of one
 * position in one run, ascending; the thread at a run's head walks the run, names every member's vertex after itself and sums
 * the vertex pseudonormal in that order.  A thread per half-edge writes its unordered vertex pair; two stable passes (the larger
 * id, then the smaller) leave the half-edges of one edge in one run; the thread at its head walks it, names the edge, classifies
 * it, sums its pseudonormal and marks its two vertices (integer OR).  A last thread per slot counts the marked vertices and
 * writes the per-record table.  No thread waits for another, no float atomics: every sum has the order of its run.
 */
#pragma once
#include "ppp_trimesh.h"

#define TT_T 256
#define TT_WORDS 8 /* the counters: vertices, edges, border, manifold, inconsistent, non-manifold edges, border, irregular vertices */

/* the topology as the kernels see it: by value.  Arrays over slots hold a vertex's or an edge's data at its id's slot. */
struct TriTopo {
    const int *rec_of;            /* [n_tris] the record of triangle f, -1: degenerate */
    const int *vslot;             /* [slots] the vertex of corner j */
    const int *eslot;             /* [slots] the edge of half-edge j */
    const unsigned char *eclass;  /* [slots] at an edge's slot: PPP_EDGE_* */
    const unsigned *vbits;        /* [slots] at a vertex's slot: PPP_VERTEX_BORDER | PPP_VERTEX_IRREGULAR */
    const double *vpn, *epn;      /* [3 slots] at a vertex's / an edge's slot: the pseudonormal */
    const int *table;             /* [6 records] the rotated frame's a, b, c, ab, ac, bc as slots */
    int n_tris;
};

__device__ inline int tt_rot(const TriRec *__restrict__ rec, int r) { return __float_as_int(rec[r].c.z); }
__device__ inline int tt_corner_id(const TriRec *__restrict__ rec, int slot) { return 3 * __float_as_int(rec[slot / 3].c.y) + slot % 3; }

/* the resident floats of the caller's corners 0, 1, 2 of record r, widened: v[k] = the rotated frame's vertex (k - rot) mod 3 */
__device__ inline void tt_corners(const TriRec *__restrict__ rec, int r, double v[3][3])
{
    double p[3][3];
    int f;
    tm_load(rec, r, p[0], p[1], p[2], &f);
    const int rot = tt_rot(rec, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k - rot + 3) % 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) v[k][d] = i == 0 ? p[0][d] : (i == 1 ? p[1][d] : p[2][d]);
    }
}

/* the oriented facet normal of record r exactly as k_mesh_nearest forms it; returns whether the orient rule negated it */
__device__ inline bool tt_facet_normal(const TriGrid &G, int r, double n[3])
{
    double a[3], b[3], c[3], N[3];
    int f;
    tm_load(G.rec, r, a, b, c, &f);
    const double A2 = tm_normal(a, b, c, N);
    n[0] = N[0] / A2; n[1] = N[1] / A2; n[2] = N[2] / A2;
    const bool flip = G.by_viewpoint && ((N[0] * (G.vp[0] - a[0]) + N[1] * (G.vp[1] - a[1])) + N[2] * (G.vp[2] - a[2])) < 0.0;
    if (flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    return flip;
}

/* alpha of corner k of record r: atan2(|u x v|, dot(u, v)), u to the next corner, v to the one before */
__device__ inline double tt_angle(const TriRec *__restrict__ rec, int r, int k)
{
    double c[3][3];
    tt_corners(rec, r, c);
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    double u[3], v[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double o = k == 0 ? c[0][d] : (k == 1 ? c[1][d] : c[2][d]);
        u[d] = (k1 == 0 ? c[0][d] : (k1 == 1 ? c[1][d] : c[2][d])) - o;
        v[d] = (k2 == 0 ? c[0][d] : (k2 == 1 ? c[1][d] : c[2][d])) - o;
    }
    const double x[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    return atan2(sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]);
}

/* a thread per slot: the coordinate keys of its corner (x + 0 turns -0 into +0; equal floats then have equal bits), the slot as
   the sort's value; corner 0 of a record writes rec_of (the array holds -1 before the launch) */
__global__ void __launch_bounds__(TT_T) k_tt_corners(const TriRec *__restrict__ rec, int slots, unsigned *__restrict__ kx, unsigned *__restrict__ ky,
                                                     unsigned *__restrict__ kz, int *__restrict__ val, int *__restrict__ rec_of)
{
    const int j = blockIdx.x * TT_T + threadIdx.x;
    if (j >= slots) return;
    const int r = j / 3, k = j % 3;
    const float4 u = rec[r].a, v = rec[r].b, w = rec[r].c;
    const int i = (k - __float_as_int(w.z) + 3) % 3;
    const float x = i == 0 ? u.x : (i == 1 ? u.w : v.z), y = i == 0 ? u.y : (i == 1 ? v.x : v.w), z = i == 0 ? u.z : (i == 1 ? v.y : w.x);
    kx[j] = __float_as_uint(x + 0.f); ky[j] = __float_as_uint(y + 0.f); kz[j] = __float_as_uint(z + 0.f);
    val[j] = j;
    if (k == 0) rec_of[__float_as_int(w.y)] = r;
}

/* the key of the next pass in the order of the last: out[i] = key[order[i]] */
__global__ void __launch_bounds__(TT_T) k_tt_gather(int n, const unsigned *__restrict__ key, const int *__restrict__ order, unsigned *__restrict__ out)
{
    const int i = blockIdx.x * TT_T + threadIdx.x;
    if (i < n) out[i] = key[order[i]];
}

/* a thread per sorted corner: the head of a run (the first corner of its position) names the run's corners after itself and sums
   alpha n_f over them in the run's order, ascending 3 f + k; cnt[0] counts the heads */
__global__ void __launch_bounds__(TT_T) k_tt_vertices(TriGrid G, int slots, const int *__restrict__ order, const unsigned *__restrict__ kx,
                                                      const unsigned *__restrict__ ky, const unsigned *__restrict__ kz, int *__restrict__ vslot,
                                                      double *__restrict__ vpn, unsigned long long *cnt)
{
    const int i = blockIdx.x * TT_T + threadIdx.x;
    unsigned long long heads = 0;
    if (i < slots) {
        const int j = order[i];
        const unsigned x = kx[j], y = ky[j], z = kz[j];
        bool head = i == 0;
        if (!head) { const int q = order[i - 1]; head = kx[q] != x || ky[q] != y || kz[q] != z; }
        if (head) {
            heads = 1;
            double s[3] = {0.0, 0.0, 0.0};
            for (int m = i; m < slots; ++m) {
                const int q = order[m];
                if (m > i && (kx[q] != x || ky[q] != y || kz[q] != z)) break;
                vslot[q] = j;
                double n[3];
                (void)tt_facet_normal(G, q / 3, n);
                const double alpha = tt_angle(G.rec, q / 3, q % 3);
                s[0] = s[0] + alpha * n[0]; s[1] = s[1] + alpha * n[1]; s[2] = s[2] + alpha * n[2];
            }
            vpn[3 * (size_t)j] = s[0]; vpn[3 * (size_t)j + 1] = s[1]; vpn[3 * (size_t)j + 2] = s[2];
        }
    }
    heads = wave_sum(heads);
    if ((threadIdx.x & 63) == 0 && heads) atomicAdd(cnt, heads);
}

/* a thread per half-edge j = 3 r + k, from corner k to corner (k + 1) % 3, reversed where the orient rule negated the facet:
   its vertex pair (lo < hi: a non-degenerate triangle has three positions), whether it runs from lo to hi, the slot as the value */
__global__ void __launch_bounds__(TT_T) k_tt_halfedges(TriGrid G, int slots, const int *__restrict__ vslot, unsigned *__restrict__ klo,
                                                       unsigned *__restrict__ khi, unsigned char *__restrict__ up, int *__restrict__ val)
{
    const int j = blockIdx.x * TT_T + threadIdx.x;
    if (j >= slots) return;
    const int r = j / 3, k = j % 3;
    int from = vslot[j], to = vslot[3 * r + (k + 1) % 3];
    double n[3];
    if (tt_facet_normal(G, r, n)) { const int t = from; from = to; to = t; }
    klo[j] = (unsigned)min(from, to); khi[j] = (unsigned)max(from, to);
    up[j] = from < to ? 1 : 0;
    val[j] = j;
}

/* a thread per sorted half-edge: the head of a run (the first half-edge of its vertex pair) names the run after itself, sums n_f
   over it in the run's order, classifies the edge and marks its two vertices; cnt[1] edges, cnt[2 + class] by class */
__global__ void __launch_bounds__(TT_T) k_tt_edges(TriGrid G, int slots, const int *__restrict__ order, const unsigned *__restrict__ klo,
                                                   const unsigned *__restrict__ khi, const unsigned char *__restrict__ up, int *__restrict__ eslot,
                                                   unsigned char *__restrict__ eclass, double *__restrict__ epn, unsigned *vbits, unsigned long long *cnt)
{
    const int i = blockIdx.x * TT_T + threadIdx.x;
    unsigned long long by[4] = {0, 0, 0, 0};
    if (i < slots) {
        const int j = order[i];
        const unsigned lo = klo[j], hi = khi[j];
        bool head = i == 0;
        if (!head) { const int q = order[i - 1]; head = klo[q] != lo || khi[q] != hi; }
        if (head) {
            double s[3] = {0.0, 0.0, 0.0};
            int count = 0, ups = 0;
            for (int m = i; m < slots; ++m) {
                const int q = order[m];
                if (m > i && (klo[q] != lo || khi[q] != hi)) break;
                eslot[q] = j;
                double n[3];
                (void)tt_facet_normal(G, q / 3, n);
                s[0] = s[0] + n[0]; s[1] = s[1] + n[1]; s[2] = s[2] + n[2];
                ++count; ups += up[q];
            }
            const int cls = count == 1 ? PPP_EDGE_BORDER : (count > 2 ? PPP_EDGE_NONMANIFOLD : (ups == 1 ? PPP_EDGE_MANIFOLD : PPP_EDGE_INCONSISTENT));
            eclass[j] = (unsigned char)cls;
            epn[3 * (size_t)j] = s[0]; epn[3 * (size_t)j + 1] = s[1]; epn[3 * (size_t)j + 2] = s[2];
            const unsigned bit = cls == PPP_EDGE_BORDER ? (unsigned)PPP_VERTEX_BORDER : (cls == PPP_EDGE_MANIFOLD ? 0u : (unsigned)PPP_VERTEX_IRREGULAR);
            if (bit) { atomicOr(vbits + lo, bit); atomicOr(vbits + hi, bit); }
#pragma unroll
            for (int c = 0; c < 4; ++c) by[c] = cls == c;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        by[c] = wave_sum(by[c]);
        if ((threadIdx.x & 63) == 0 && by[c]) { atomicAdd(cnt + 2 + c, by[c]); atomicAdd(cnt + 1, by[c]); }
    }
}

/* a thread per slot: a vertex's own slot counts its bits (cnt[6] border, cnt[7] irregular); corner 0 of a record writes the
   record's table in the rotated frame, a cyclic shift of the caller's: a = corner rot, ab = half-edge rot, bc the next, ac (c to
   a) the one after */
__global__ void __launch_bounds__(TT_T) k_tt_table(const TriRec *__restrict__ rec, int slots, const int *__restrict__ vslot, const int *__restrict__ eslot,
                                                   const unsigned *__restrict__ vbits, int *__restrict__ table, unsigned long long *cnt)
{
    const int j = blockIdx.x * TT_T + threadIdx.x;
    unsigned long long border = 0, irregular = 0;
    if (j < slots) {
        if (vslot[j] == j) { border = (vbits[j] & PPP_VERTEX_BORDER) != 0; irregular = (vbits[j] & PPP_VERTEX_IRREGULAR) != 0; }
        if (j % 3 == 0) {
            const int r = j / 3, rot = tt_rot(rec, r);
            const int k0 = 3 * r + rot, k1 = 3 * r + (rot + 1) % 3, k2 = 3 * r + (rot + 2) % 3;
            int *t = table + 6 * (size_t)r;
            t[0] = vslot[k0]; t[1] = vslot[k1]; t[2] = vslot[k2];
            t[3] = eslot[k0]; t[4] = eslot[k2]; t[5] = eslot[k1];
        }
    }
    border = wave_sum(border); irregular = wave_sum(irregular);
    if ((threadIdx.x & 63) == 0 && border) atomicAdd(cnt + 6, border);
    if ((threadIdx.x & 63) == 0 && irregular) atomicAdd(cnt + 7, irregular);
}

/* a thread per triangle of the caller's list below cap: its three corners' rows of ppp_trimesh_get_topology's maps */
__global__ void __launch_bounds__(TT_T) k_tt_export(const TriRec *__restrict__ rec, TriTopo T, int cap, int *__restrict__ vertex_id, int *__restrict__ edge_id,
                                                    unsigned char *__restrict__ edge_class, unsigned char *__restrict__ vertex_bits,
                                                    double *__restrict__ vertex_normal, double *__restrict__ edge_normal)
{
    const int f = blockIdx.x * TT_T + threadIdx.x;
    if (f >= cap) return;
    const int r = T.rec_of[f];
    for (int k = 0; k < 3; ++k) {
        const size_t o = 3 * (size_t)f + k;
        if (r < 0) {
            vertex_id[o] = -1; edge_id[o] = -1; edge_class[o] = 255; vertex_bits[o] = 255;
            for (int d = 0; d < 3; ++d) { vertex_normal[3 * o + d] = dev_nan(); edge_normal[3 * o + d] = dev_nan(); }
            continue;
        }
        const int v = T.vslot[3 * r + k], e = T.eslot[3 * r + k];
        vertex_id[o] = tt_corner_id(rec, v); edge_id[o] = tt_corner_id(rec, e);
        edge_class[o] = T.eclass[e]; vertex_bits[o] = (unsigned char)T.vbits[v];
        for (int d = 0; d < 3; ++d) { vertex_normal[3 * o + d] = T.vpn[3 * (size_t)v + d]; edge_normal[3 * o + d] = T.epn[3 * (size_t)e + d]; }
    }
}

/* tm_closest with the feature beside the region: the same inputs, the same arithmetic in the same order, so x, D2 and the region
   are tm_closest's bits.  *feature, in the rotated frame: 0 a, 1 b, 2 c, 3 ab, 4 ac, 5 bc, 6 the face. */
__device__ __attribute__((always_inline)) inline int tm_closest_feature(const double p[3], const double a[3], const double b[3], const double c[3], double x[3],
                                                                        double *D2, int *feature)
{
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    auto dot = [](const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; };
    int region, feat = 6;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    double d3 = 0.0, d4 = 0.0, d5 = 0.0, d6 = 0.0, vc = 0.0, vb = 0.0, va = 0.0;
    bool done = false;
    if (d1 <= 0.0 && d2 <= 0.0) { x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; region = 2; feat = 0; done = true; }
    if (!done) {
        const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
        d3 = dot(ab, bp); d4 = dot(ac, bp);
        if (d3 >= 0.0 && d4 <= d3) { x[0] = b[0]; x[1] = b[1]; x[2] = b[2]; region = 2; feat = 1; done = true; }
    }
    if (!done) {
        vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double v = d1 / (d1 - d3);
            x[0] = a[0] + ab[0] * v; x[1] = a[1] + ab[1] * v; x[2] = a[2] + ab[2] * v; region = 1; feat = 3; done = true;
        }
    }
    if (!done) {
        const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
        d5 = dot(ab, cp); d6 = dot(ac, cp);
        if (d6 >= 0.0 && d5 <= d6) { x[0] = c[0]; x[1] = c[1]; x[2] = c[2]; region = 2; feat = 2; done = true; }
    }
    if (!done) {
        vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
            x[0] = a[0] + ac[0] * w; x[1] = a[1] + ac[1] * w; x[2] = a[2] + ac[2] * w; region = 1; feat = 4; done = true;
        }
    }
    if (!done) {
        va = d3 * d6 - d5 * d4;
        if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
            const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
            x[0] = b[0] + (c[0] - b[0]) * w; x[1] = b[1] + (c[1] - b[1]) * w; x[2] = b[2] + (c[2] - b[2]) * w; region = 1; feat = 5;
        } else {
            const double den = 1.0 / ((va + vb) + vc), v = vb * den, w = vc * den;
            x[0] = (a[0] + ab[0] * v) + ac[0] * w; x[1] = (a[1] + ab[1] * v) + ac[1] * w; x[2] = (a[2] + ab[2] * v) + ac[2] * w; region = 0;
        }
    }
    const double ex = p[0] - x[0], ey = p[1] - x[1], ez = p[2] - x[2];
    *D2 = (ex * ex + ey * ey) + ez * ez;
    *feature = feat;
    return region;
}

/* The sign kernel: one thread per query, behind k_mesh_nearest with the same queries (q4 / xyz as there).  It reads the status
   and the winner that launch wrote, reloads the winner's record, walks that one triangle again and looks the feature's
   pseudonormal up.  signed_distance and status / tri_index are required; pseudonormal, feature, flags are optional; dev, fix
   (ppp_get_mesh_signed_deviation's): the deviation map and its fixed-point term are rewritten with the signed distance. */
struct TmSignOut {
    double *signed_distance, *pseudonormal, *dev;
    long long *fix;
    unsigned char *feature, *flags;
    const int *tri_index;
    const unsigned char *status;
};

/* k_mesh_sign's body for one query whose entries go to `id`: the whole-cloud kernel and the tile form (k_mesht_sign,
   ppp_mesh_tile.h) call it: equal bits from equal code. */
__device__ __forceinline__ void mesh_sign_body(float qx, float qy, float qz, int id, const TriGrid &G, const TriTopo &T, const TmSignOut &O)
{
    const int f = O.status[id] == PPP_DEV_MATCHED ? O.tri_index[id] : -1;
    const int r = f >= 0 && f < T.n_tris ? T.rec_of[f] : -1;
    double sd = dev_nan(), g[3] = {dev_nan(), dev_nan(), dev_nan()};
    int feature = 255, flags = 0;
    if (r >= 0) {
        const double p[3] = {(double)qx, (double)qy, (double)qz};
        double a[3], b[3], c[3], x[3], n[3], D2;
        int ff, feat;
        tm_load(G.rec, r, a, b, c, &ff);
        (void)tm_closest_feature(p, a, b, c, x, &D2, &feat);
        (void)tt_facet_normal(G, r, n);
        const double e[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
        const double dev = ((e[0] * n[0]) + e[1] * n[1]) + e[2] * n[2];
        const int rot = tt_rot(G.rec, r);
        if (feat == 6) { g[0] = n[0]; g[1] = n[1]; g[2] = n[2]; feature = 6; }
        else {
            const int s = T.table[6 * (size_t)r + feat];
            const double *src = (feat < 3 ? T.vpn : T.epn) + 3 * (size_t)s;
            g[0] = src[0]; g[1] = src[1]; g[2] = src[2];
            if (feat < 3) {
                flags = (int)(T.vbits[s] & 3u); /* (PPP_VERTEX_* are PPP_MESH_SIGN_BORDER and _IRREGULAR) */
                feature = (feat + rot) % 3;
            } else {
                const int cls = T.eclass[s];
                flags = cls == PPP_EDGE_BORDER ? PPP_MESH_SIGN_BORDER : (cls == PPP_EDGE_MANIFOLD ? 0 : PPP_MESH_SIGN_IRREGULAR);
                feature = 3 + (rot + (feat == 3 ? 0 : (feat == 5 ? 1 : 2))) % 3; /* ab, bc, ca are the caller's half-edges rot, rot + 1, rot + 2 */
            }
        }
        const double s = (e[0] * g[0] + e[1] * g[1]) + e[2] * g[2];
        const double dist = sqrt(D2);
        const bool zero = g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0;
        if ((s > 0.0 || s < 0.0) && !zero) sd = copysign(dist, s);
        else { sd = copysign(dist, dev); flags |= PPP_MESH_SIGN_FALLBACK; }
    }
    O.signed_distance[id] = sd;
    if (O.pseudonormal) { double *o = O.pseudonormal + 3 * (size_t)id; o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; }
    if (O.feature) O.feature[id] = (unsigned char)feature;
    if (O.flags) O.flags[id] = (unsigned char)flags;
    if (r >= 0 && O.dev) O.dev[id] = sd;
    if (r >= 0 && O.fix) O.fix[id] = llrint(sd * DEV_FIXED);
}

__global__ void __launch_bounds__(TM_T) k_mesh_sign(const float4 *__restrict__ q4, const float *__restrict__ xyz, int nq, const TriGrid G, const TriTopo T, TmSignOut O)
{
    const int t = blockIdx.x * TM_T + threadIdx.x;
    if (t >= nq) return;
    float qx, qy, qz;
    int id = t;
    if (q4) { const float4 q = q4[t]; qx = q.x; qy = q.y; qz = q.z; id = idx_of(q); }
    else { qx = xyz[3 * (size_t)t]; qy = xyz[3 * (size_t)t + 1]; qz = xyz[3 * (size_t)t + 2]; }
    mesh_sign_body(qx, qy, qz, id, G, T, O);
}

/* what the signed maps hold where the sign kernel does not write (points outside the slab index): a thread per cloud index */
__global__ void __launch_bounds__(TM_T) k_tm_sign_fill(int n, unsigned char *__restrict__ feature, unsigned char *__restrict__ flags)
{
    for (int i = blockIdx.x * TM_T + threadIdx.x; i < n; i += gridDim.x * TM_T) { feature[i] = 255; flags[i] = 0; }
}

/* the matched points by flag and by sign: acc[0] border, [1] irregular, [2] fallback, [3] negative (< 0), [4] positive (> 0) */
__global__ void __launch_bounds__(TM_T) k_tm_sign_stats(int n, const unsigned char *__restrict__ status, const unsigned char *__restrict__ flags,
                                                        const double *__restrict__ signed_distance, unsigned long long *acc)
{
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    for (int i = blockIdx.x * TM_T + threadIdx.x; i < n; i += gridDim.x * TM_T) {
        if (status[i] != PPP_DEV_MATCHED) continue;
        const int fl = flags[i];
        const double v = signed_distance[i];
        cnt[0] += (fl & PPP_MESH_SIGN_BORDER) != 0; cnt[1] += (fl & PPP_MESH_SIGN_IRREGULAR) != 0; cnt[2] += (fl & PPP_MESH_SIGN_FALLBACK) != 0;
        cnt[3] += v < 0.0; cnt[4] += v > 0.0;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        cnt[k] = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && cnt[k]) atomicAdd(acc + k, cnt[k]);
    }
}
