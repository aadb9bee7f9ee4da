/*
 * ppp_query_host.h -- the host helpers that both query units call, ppp_contact.hip and ppp_scan.hip: the kernels' view of a
 * handle's index, the normal field behind an index, the partition of a map for a fixed-order sum, and what a slice-range
 * handle's tile owns, evaluates and indexes.  Static: each unit has its own copy, the diagnostic single-unit build sees them once.
 */
#pragma once
#include "ppp_handle.h"
#include "ppp_contact.h"

/* the kernels' view of the handle's slab index / normal field, as it stands when the launch is made */
static inline ContactIndex contact_index(const ppp_handle h)
{
    return ContactIndex{h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_xmin.p, h->slab_xmax.p, h->normals4.p, h->ell_cs.p, h->slab_ytab.p};
}

/* A finished pass with the dynamic adjustment left the normal field of THIS cloud and THESE parameters in normals4: every
   ppp_set_params and every cloud change plans again, which withdraws gen_done (a changed normal_radius included).  The
   contact queries then skip the launch; ppp_area2cloud, older than they are, builds the field every time and is left as it was. */
static inline bool pass_left_normals(const ppp_handle h) { return h->pass.gen_done() && h->P.dynamic_adjustment; }

/* behind index_ready: the Area2Cloud buffers and the normal field (a pass with the dynamic adjustment made it) */
static inline int contact_buffers(ppp_handle h)
{
    int rc = ensure_dynamic_buffers(h);
    if (rc) return rc;
    return pass_left_normals(h) ? PPP_OK : enqueue_normals(h);
}

/* The partition of a map of N entries for a fixed-order sum (B.46, block_tree_sum): workgroup g of grid takes [g per, (g + 1) per);
   the host adds the workgroups' parts in order */
struct MapParts {
    int grid, per;
    MapParts(const ppp_handle h, size_t N)
        : grid((int)std::max<size_t>(1, std::min<size_t>((N + PCON_T - 1) / PCON_T, 2 * (size_t)h->num_cus))), per((int)((N + grid - 1) / grid)) {}
};

/* What this handle's tile evaluates and owns, behind a plan: the cuts of its range [sb, se) on the walk of the
   whole cloud's bounds, widened by halo; a whole-cloud handle owns and evaluates everything. */
static inline int tile_range(ppp_handle h, float halo, TileRange &T)
{
    T = TileRange{-INFINITY, INFINITY, -INFINITY, INFINITY};
    if (!h->ranged) return PPP_OK;
    const int S = h->S_cap;
    std::vector<float> px((size_t)S);
    if (ppp_slice_walk(h->P.walk, h->h_mn[0], h->h_mx[0], h->P.tool_radius, px.data(), S) != S) return fail(h, PPP_ERR_HIP, "tile: the slice walk changed under the plan");
    owned_cuts(px.data(), S, h->sb, h->se, &T.own_lo, &T.own_hi);
    T.ev_lo = T.own_lo - halo; T.ev_hi = T.own_hi + halo;
    return PPP_OK;
}

/* does the interval [lo, hi] leave what the handle indexes at a side that is not the cloud's end? (wave_ball_leaves_range's test) */
static inline bool leaves_indexed_range(const ppp_handle h, float lo, float hi)
{
    return h->ranged && lo <= hi && ((lo < h->incl_lo && h->incl_lo > h->h_mn[0]) || (hi > h->incl_hi && h->incl_hi < h->h_mx[0]));
}

/* the positions [pos0, pos1) of the slabs that meet the tile's evaluated interval (one slab more on either side: the kernels
   test every point themselves), behind index_ready */
static inline int tile_positions(ppp_handle h, const TileRange &T, int &pos0, int &pos1)
{
    pos0 = pos1 = 0;
    const int ns = h->hmeta.n_sorted;
    if (ns < 0 || (size_t)ns > h->n) return fail(h, PPP_ERR_HIP, "tile: index corrupt");
    if (!(T.ev_lo <= T.ev_hi) || ns == 0) return PPP_OK;
    const SlabGeom G = slab_geom(h);
    auto slab_of_host = [&](float x) { return (int)fminf(fmaxf((x - G.slab_x0) * G.slab_invw, 0.f), (float)(h->B - 1)); };
    const int b0 = std::max(0, slab_of_host(T.ev_lo) - 1), b1 = std::min(h->B - 1, slab_of_host(T.ev_hi) + 1);
    HIPCHK(h, copy_sync(h, &pos0, h->slab_start.p + b0, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, &pos1, h->slab_start.p + b1 + 1, sizeof(int), hipMemcpyDeviceToHost));
    if (pos0 < 0 || pos1 < pos0 || pos1 > ns) return fail(h, PPP_ERR_HIP, "tile: slab table corrupt");
    return PPP_OK;
}
