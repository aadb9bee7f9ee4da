/*
 * ppp_scan.hip -- the calls of the C ABI (include/ppp_hip.h) that hold a scan against a reference cloud: the deviation map, its
 * tiles and their merge, the registration chain, its trimmed and its robust form, the cloud moments and the global registration,
 * the registration, the trimmed and the robust registration of a scan held as slice-range tiles, and the resident triangle mesh
 * with its exact point-to-triangle search and deviation map (ppp_trimesh.h).  The unit owns the kernels of ppp_deviation.h,
 * ppp_deviation_tile.h, ppp_registration.h, ppp_trimmed.h, ppp_robust.h, ppp_registration_tile.h, ppp_trimmed_tile.h and ppp_robust_tile.h; of the handle it sees
 * what ppp_handle.h declares, and it shares ppp_query_host.h with ppp_contact.hip.  Compiled with the engine's flags: the host
 * and the device step share icp_solve and icp_compose, one IEEE rounding per written operation on both sides.
 */
#ifndef PPP_SINGLE_TU /* (a diagnostic build includes this file into the engine's unit) */
#define PPP_KERNELS_FOREIGN /* ppp_kernels.h, ppp_dynamic.h, ppp_compact.h: types and device helpers only -- their kernels are the engine's */
#define PPP_CONTACT_KERNELS_FOREIGN /* ppp_contact.h likewise: its kernels are ppp_contact.hip's */
#define PPP_MESH_KERNELS_FOREIGN /* ppp_mesh.h likewise: the sampler's kernels are ppp_preproc.hip's */
#endif
#include "ppp_query_host.h"
#include "ppp_deviation.h"
#include "ppp_deviation_tile.h"
#include "ppp_registration.h"
#include "ppp_trimmed.h"
#include "ppp_robust.h"
#include "ppp_registration_tile.h"
#include "ppp_trimmed_tile.h"
#include "ppp_robust_tile.h"
#include "ppp_trimesh.h"
#include "ppp_trimesh_topology.h"
#include "ppp_mesh_registration.h"
#include "ppp_mesh_robust.h"
#include "ppp_mesh_trimmed.h"
#include "ppp_mesh_tile.h"
#include "ppp_sort.h"
#include <cstring>
#include <mutex>

/* what the deviation accumulator words [0 .. 9] say in the whole-cloud call's statistics or a tile's (a template: C++ linkage) */
template <typename Stats>
static void dev_stats_words(Stats &st, size_t N, const unsigned long long *acc)
{
    st.n = N; st.matched = (size_t)acc[0]; st.too_far = (size_t)acc[1]; st.no_normal = (size_t)acc[2];
    st.proud = (size_t)acc[DEV_ACC_PROUD]; st.below = (size_t)acc[DEV_ACC_BELOW];
    st.min_dev = st.max_dev = (double)NAN; st.max_dist2 = NAN;
    if (!st.matched) return;
    st.min_dev = -ordered_unkey64(acc[DEV_ACC_NMIN]); st.max_dev = ordered_unkey64(acc[DEV_ACC_MAX]);
    st.max_dist2 = ordered_unkey((unsigned)acc[DEV_ACC_D2]);
}

extern "C" {

void ppp_default_deviation_params(ppp_deviation_params *dp)
{
    if (!dp) return;
    dp->max_dist = INFINITY; dp->smooth_radius = 0.f; dp->allowance = 0.0; dp->gain = 1.0;
}

/* The checks of a scan-against-reference call's handle, scan or reference (w: "<call>: <which handle>"); refusals and errors are
   reported on h, the call's first argument, whichever handle they are about.  deviation_side_cloud builds no index and launches
   nothing (plan: the tile call's, whose range checks want what the handle owns); deviation_side_index builds the slab index. */
static int deviation_side_cloud(ppp_handle h, ppp_handle side, const std::string &w, bool plan)
{
    if (!side->have_cloud) return fail(h, PPP_ERR_ARG, w + " holds no cloud");
    if (side->part_given) return fail(h, PPP_ERR_UNSUPPORTED, w + " holds a part (ppp_set_cloud_part): the maps address the whole cloud");
    const int rc = plan ? plan_ready(side) : PPP_OK;
    return rc && side != h ? fail(h, rc, w + ": " + side->err) : rc;
}
static int deviation_side_index(ppp_handle h, ppp_handle side, const std::string &w, bool whole)
{
    int rc = index_ready(side, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
    if (rc) return side == h ? rc : fail(h, rc, w + ": " + side->err);
    if (whole && (side->ranged || side->use_part)) return fail(h, PPP_ERR_UNSUPPORTED, w + " is a slice-range handle: it indexes a part of the cloud only");
    const int ns = side->hmeta.n_sorted;
    if (side->n > 0x7fffffffu || ns < 0 || (size_t)ns > side->n) return fail(h, PPP_ERR_HIP, w + ": index corrupt");
    return PPP_OK;
}
/* a handle of ppp_get_deviation, scan or reference: a cloud, all of it, its slab index complete */
static int deviation_side(ppp_handle h, ppp_handle side, const char *who, const char *what = "deviation")
{
    const std::string w = std::string(what) + ": " + who;
    int rc = deviation_side_cloud(h, side, w, false);
    if (rc) return rc;
    if (side->P.slice_begin != 0 || side->P.slice_end != 0) return fail(h, PPP_ERR_UNSUPPORTED, w + " is a slice-range handle: it indexes a part of the cloud only");
    return deviation_side_index(h, side, w, true);
}

/* both deviation calls' checks before they look at a handle, in the order they fire; w: the call's name, halo: the tile call's */
static int deviation_params_ok(ppp_handle h, const ppp_deviation_params &P, const std::string &w, const float *halo);
static int deviation_call_ok(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp, const std::string &w, const float *halo)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!ref || !dp) return fail(h, PPP_ERR_ARG, w + ": no reference handle or no parameters");
    const int rc = deviation_params_ok(h, *dp, w, halo);
    if (rc) return rc;
    if (ref->device != h->device) return fail(h, PPP_ERR_ARG, w + ": the two handles are on different devices");
    return PPP_OK;
}
/* ... those of them that read the parameters alone (the mesh call's too: it has no reference handle) */
static int deviation_params_ok(ppp_handle h, const ppp_deviation_params &P, const std::string &w, const float *halo)
{
    if (!(P.max_dist > 0.f)) return fail(h, PPP_ERR_ARG, w + (halo ? ": max_dist must be > 0" : ": max_dist must be > 0 (+INFINITY: no limit)"));
    if (halo && !std::isfinite(P.max_dist)) return fail(h, PPP_ERR_ARG, w + ": a tile needs a finite max_dist: the halo must hold every partner");
    if (!(P.smooth_radius >= 0.f && std::isfinite(P.smooth_radius))) return fail(h, PPP_ERR_ARG, w + ": smooth_radius must be finite and >= 0");
    if (!std::isfinite(P.allowance)) return fail(h, PPP_ERR_ARG, w + ": allowance must be finite");
    if (!(P.gain >= 0.0 && std::isfinite(P.gain))) return fail(h, PPP_ERR_ARG, w + ": gain must be finite and >= 0");
    if (!halo && P.smooth_radius > 0.f && !std::isfinite(P.max_dist)) return fail(h, PPP_ERR_ARG, w + ": smoothing needs a finite max_dist");
    if (halo && !(*halo >= P.max_dist + P.smooth_radius && *halo <= 3.402823466e+38f))
        return fail(h, PPP_ERR_ARG, w + ": halo must be finite and at least max_dist + smooth_radius");
    return PPP_OK;
}

/* the integer sum of a neighbourhood or of the statistics: |deviation| <= about max_dist, n terms of it in 2^-24 mm */
static bool deviation_sum_overflows(const ppp_deviation_params &P, size_t n) { return P.smooth_radius > 0.f && (double)P.max_dist * DEV_FIXED * (double)n >= 4611686018427387904.0; }

/* the reference's normal field, on ref's stream, and the one wait for that stream */
static int reference_normals(ppp_handle h, ppp_handle ref, const char *what)
{
    int rc = contact_buffers(ref);
    if (rc) return ref == h ? rc : fail(h, rc, std::string(what) + ": the reference: " + ref->err);
    if (ref != h) HIPCHK(h, hipStreamSynchronize(ref->stream));
    return PPP_OK;
}

/* the maps' first k entries to the caller's arrays, those it gave (owned: the tile call's, behind the five maps) */
static int deviation_copy_out(ppp_handle h, size_t k, const double *v, double *deviation, double *smoothed, int *ref_index, unsigned char *status, double *target,
                              unsigned char *owned = nullptr)
{
    auto &D = h->deviation;
    if (deviation && k) HIPCHK(h, copy_sync(h, deviation, D.dev.p, k * sizeof(double), hipMemcpyDeviceToHost));
    if (smoothed && k) HIPCHK(h, copy_sync(h, smoothed, v, k * sizeof(double), hipMemcpyDeviceToHost));
    if (ref_index && k) HIPCHK(h, copy_sync(h, ref_index, D.ref_index.p, k * sizeof(int), hipMemcpyDeviceToHost));
    if (status && k) HIPCHK(h, copy_sync(h, status, D.status.p, k, hipMemcpyDeviceToHost));
    if (target && k) HIPCHK(h, copy_sync(h, target, D.target.p, k * sizeof(double), hipMemcpyDeviceToHost));
    if (owned && k) HIPCHK(h, copy_sync(h, owned, D.owned.p, k, hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* The tail of a deviation call behind its search (ppp_get_mesh_deviation runs it too): status, deviation, its
   fixed-point term and the float d2 are in h's buffers and the accumulators are clear; k_dev_smooth where asked, k_dev_target
   and k_dev_stats on the scan's stream, the one wait, and the statistics.  *v: the map the target was taken from. */
static int deviation_tail(ppp_handle h, const ppp_deviation_params &P, const MapParts &parts, const char *what, ppp_deviation_stats *stats, const double **v_out)
{
    auto &D = h->deviation;
    const bool smooth = P.smooth_radius > 0.f;
    const size_t N = h->n, N1 = std::max<size_t>(N, 1);
    const int grid = parts.grid, per = parts.per, nq = h->hmeta.n_sorted;
    double *v = smooth ? D.smoothed.p : D.dev.p;
    if (nq > 0 && smooth)
        LAUNCH(h, "k_dev_smooth", k_dev_smooth, (unsigned)((nq + DEV_T - 1) / DEV_T), DEV_T, 0, contact_index(h), nq, P.smooth_radius * P.smooth_radius, D.status.p,
               D.fix.p, D.smoothed.p);
    LAUNCH(h, "k_dev_target", k_dev_target, (unsigned)std::min<size_t>((N1 + DEV_T - 1) / DEV_T, 2 * (size_t)h->num_cus), DEV_T, 0, D.status.p,
           D.dev.p, v, D.d2.p, (int)N, P.allowance, P.gain, D.target.p, D.acc.p);
    LAUNCH(h, "k_dev_stats", k_dev_stats, (unsigned)grid, PCON_T, 0, D.status.p, v, D.target.p, (int)N, per, D.acc.p, D.psum.p, D.psum.p + grid);
    unsigned long long acc[DEV_ACC_WORDS];
    std::vector<double> psum(2 * (size_t)grid);
    HIPCHK(h, copy_sync(h, acc, D.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
    HIPCHK(h, copy_sync(h, psum.data(), D.psum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (acc[0] + acc[1] + acc[2] + acc[3] != N || acc[DEV_ACC_PROUD] > acc[0] || acc[DEV_ACC_BELOW] > acc[0])
        return fail(h, PPP_ERR_HIP, std::string(what) + ": statistics corrupt");
    if (stats) {
        ppp_deviation_stats st = {};
        dev_stats_words(st, N, acc);
        st.dropped = (size_t)acc[3];
        double sq = 0.0;
        for (int g = 0; g < grid; ++g) { sq += psum[(size_t)g]; st.target_sum += psum[(size_t)grid + g]; }
        st.mean_dev = st.matched ? (double)(long long)acc[DEV_ACC_FIXSUM] / (double)st.matched * (1.0 / DEV_FIXED) : (double)NAN;
        st.rms_dev = st.matched ? std::sqrt(sq / (double)st.matched) : (double)NAN;
        for (int b = 0; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[DEV_ACC_BINS + b];
        *stats = st;
    }
    *v_out = v;
    return PPP_OK;
}

/* The deviation map: the reference's index and normal field on its own stream, one wait for that stream, then
   k_dev_nearest, k_dev_smooth where asked, k_dev_target and k_dev_stats back to back on the scan's stream, and one wait. */
int ppp_get_deviation(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp, double *deviation, double *smoothed, int *ref_index,
                      unsigned char *status, double *target, size_t cap, ppp_deviation_stats *stats)
{
    int rc = deviation_call_ok(h, ref, dp, "deviation", nullptr);
    if (rc) return rc;
    const ppp_deviation_params P = *dp;
    const bool smooth = P.smooth_radius > 0.f;
    rc = deviation_side(h, ref, "the reference");
    if (rc) return rc;
    if (ref != h) { rc = deviation_side(h, h, "the scan"); if (rc) return rc; }
    const size_t N = h->n;
    if (deviation_sum_overflows(P, N)) return fail(h, PPP_ERR_ARG, "deviation: max_dist 2^24 n reaches 2^62: the smoothing's integer sum could overflow");
    rc = reference_normals(h, ref, "deviation");
    if (rc) return rc;
    auto &D = h->deviation;
    const size_t N1 = std::max<size_t>(N, 1);
    const MapParts parts(h, N);
    const int grid = parts.grid, nq = h->hmeta.n_sorted, nref = ref->hmeta.n_sorted;
    HIPCHK(h, D.dev.ensure(N1)); HIPCHK(h, D.target.ensure(N1)); HIPCHK(h, D.fix.ensure(N1)); HIPCHK(h, D.d2.ensure(N1));
    HIPCHK(h, D.ref_index.ensure(N1)); HIPCHK(h, D.status.ensure(N1)); HIPCHK(h, D.acc.ensure(DEV_ACC_WORDS)); HIPCHK(h, D.psum.ensure(2 * (size_t)grid));
    if (smooth) HIPCHK(h, D.smoothed.ensure(N1));
    HIPCHK(h, hipMemsetAsync(D.status.p, PPP_DEV_DROPPED, N1, h->stream)); /* points outside the index: not finite */
    HIPCHK(h, hipMemsetAsync(D.ref_index.p, 0xff, N1 * sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(D.acc.p, 0, DEV_ACC_WORDS * sizeof(unsigned long long), h->stream));
    if (nq > 0)
        LAUNCH(h, "k_dev_nearest", k_dev_nearest, (unsigned)((nq + DEV_T - 1) / DEV_T), DEV_T, 0, h->sorted4.p, nq, contact_index(ref), nref, P.max_dist * P.max_dist,
               D.dev.p, D.fix.p, D.d2.p, D.ref_index.p, D.status.p);
    const double *v = nullptr;
    rc = deviation_tail(h, P, parts, "deviation", stats, &v);
    if (rc) return rc;
    return deviation_copy_out(h, std::min(cap, N), v, deviation, smoothed, ref_index, status, target);
}

void ppp_default_registration_params(ppp_registration_params *rp)
{
    if (!rp) return;
    rp->max_dist = 2.f; rp->iterations = 30; rp->min_step = 1e-6; rp->lock_eps = 1e-9;
}

/* a chain's parameters, checked; F takes what they set */
static int registration_params_ok(ppp_handle h, const ppp_registration_params &P, IcpFrame &F)
{
    F.md2 = P.max_dist * P.max_dist;
    if (!(P.max_dist > 0.f && std::isfinite(P.max_dist) && std::isfinite(F.md2)))
        return fail(h, PPP_ERR_ARG, "registration: max_dist must be finite and > 0 (and so its float square)");
    if (P.iterations < 1 || P.iterations > 64) return fail(h, PPP_ERR_ARG, "registration: iterations must be in [1, 64]");
    if (!(P.min_step >= 0.0 && std::isfinite(P.min_step))) return fail(h, PPP_ERR_ARG, "registration: min_step must be finite and >= 0");
    if (!(P.lock_eps > 0.0 && P.lock_eps < 1.0)) return fail(h, PPP_ERR_ARG, "registration: lock_eps must be in (0, 1)");
    F.lock_eps = P.lock_eps; F.min_step2 = P.min_step * P.min_step;
    return PPP_OK;
}

/* The frame a cloud's bounds imply (B.67, B.68): the box's centre, half the sum of its extents widened by max_dist, and the
   scale of the integer sums.  The order of the operations is part of the result: every caller's bits come from here. */
static void frame_from_bounds(const float *mn, const float *mx, double max_dist, int shift, double *c, double *length, double *scale)
{
    double ext[3];
    for (int d = 0; d < 3; ++d) {
        c[d] = ((double)mn[d] + (double)mx[d]) * 0.5;
        ext[d] = (double)mx[d] - (double)mn[d];
    }
    *length = (((ext[0] + ext[1]) + ext[2]) * 0.5) + max_dist;
    *scale = std::ldexp(1.0, shift);
}

/* the transform a chain or a tiled call opens with: T0, the identity where there is none; every entry finite (w: the call's name) */
static const double ICP_IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
static int opening_transform(ppp_handle h, const char *w, const double *T0, double *T)
{
    memcpy(T, T0 ? T0 : ICP_IDENTITY, sizeof(ICP_IDENTITY));
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) return fail(h, PPP_ERR_ARG, std::string(w) + ": the transform has an entry that is not finite");
    return PPP_OK;
}

/* what a chain needs before its first launch: both handles' indices, the rest of F (B.67) and the shift (B.68), the reference's
   normal field on its own stream and one wait for that stream */
static int registration_setup(ppp_handle h, ppp_handle ref, const ppp_registration_params &P, IcpFrame &F, int &shift)
{
    if (ref->device != h->device) return fail(h, PPP_ERR_ARG, "registration: the two handles are on different devices");
    int rc = deviation_side(h, ref, "the reference", "registration");
    if (rc) return rc;
    if (ref != h) { rc = deviation_side(h, h, "the scan", "registration"); if (rc) return rc; }
    rc = fetch_meta(ref);
    if (rc) return ref == h ? rc : fail(h, rc, std::string("registration: the reference: ") + ref->err);
    shift = icp_shift(h->n, F.md2);
    if (shift < 16) return fail(h, PPP_ERR_ARG, "registration: fewer than 16 fractional bits are left (n max_dist^2 too large): the integer sums could overflow");
    frame_from_bounds(ref->hmeta.mn, ref->hmeta.mx, (double)P.max_dist, shift, F.c, &F.Ln, &F.scale);
    return reference_normals(h, ref, "registration");
}

static_assert(sizeof(IcpCtl) == 5 * sizeof(int), "IcpCtl is five ints");
/* a chain's control words behind the one wait: 0 <= steps <= iterations, and a chain that has not ended took every step */
static bool chain_ctl_ok(const IcpCtl &c, int iterations) { return c.steps >= 0 && c.steps <= iterations && (c.done || c.steps == iterations); }

/* ppp_register's statistics from the rows R[0 .. C.steps] of a chain or a tiled loop, its counts, shift and frame */
static ppp_registration_stats registration_stats(const std::vector<ppp_registration_row> &R, const IcpCtl &C, size_t n, size_t indexed, int shift,
                                                 const double *centre, double length)
{
    const size_t last = (size_t)C.steps;
    ppp_registration_stats st = {};
    st.n = n; st.indexed = indexed;
    st.steps = C.steps; st.converged = C.converged; st.locked = C.locked; st.shift = shift;
    for (int d = 0; d < 3; ++d) st.centre[d] = centre[d];
    st.length = length;
    memcpy(st.T, R[last].T, sizeof(st.T));
    auto rms = [&](const ppp_registration_row &r) {
        return r.pairs ? std::sqrt(std::ldexp((double)r.E, -shift) / (double)r.pairs) : (double)NAN;
    };
    st.pairs_before = R[0].pairs; st.rms_before = rms(R[0]);
    st.pairs_after = R[last].pairs; st.rms_after = rms(R[last]);
    return st;
}

/* a row of a trimmed chain or loop as the caller gets it: the row, the pairs the search found, the cut's bits as a float */
static void trimmed_row(ppp_trimmed_registration_row &o, const ppp_registration_row &r, size_t paired, unsigned tau)
{
    memset(&o, 0, sizeof(o)); /* the padding too: rows compare as bytes */
    o.row = r;
    o.paired = paired;
    memcpy(&o.trim_d2, &tau, sizeof(float));
}

/* What ppp_register's chain and ppp_register_mesh's have in common on either side of their launches.  chain_open: room for
   `evals` evaluations in h->registration's buffers, the words and the control block cleared on h's stream, T at the chain's head.
   chain_collect: the one wait, the control words' and the sums' sanity checks (w: the call's name), and the rows R[0 .. C.steps],
   the last of them from the evaluation no step kernel follows where the chain used up its iterations. */
static int chain_open(ppp_handle h, size_t evals, const double *T)
{
    auto &G = h->registration;
    HIPCHK(h, G.T.ensure(12 * evals)); HIPCHK(h, G.acc.ensure(ICP_WORDS * evals)); HIPCHK(h, G.rows.ensure(evals)); HIPCHK(h, G.ctl.ensure(8));
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, ICP_WORDS * evals * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(G.ctl.p, 0, 8 * sizeof(int), h->stream));
    HIPCHK(h, copy_sync(h, G.T.p, T, 12 * sizeof(double), hipMemcpyHostToDevice));
    return PPP_OK;
}

static int chain_collect(ppp_handle h, const char *w, int iterations, int nq, IcpCtl &C, std::vector<ppp_registration_row> &R)
{
    auto &G = h->registration;
    HIPCHK(h, copy_sync(h, &C, G.ctl.p, sizeof(C), hipMemcpyDeviceToHost)); /* the one wait */
    if (!chain_ctl_ok(C, iterations)) return fail(h, PPP_ERR_HIP, std::string(w) + ": control words corrupt");
    const size_t last = (size_t)C.steps;
    R.resize(last + 1);
    HIPCHK(h, copy_sync(h, R.data(), G.rows.p, (last + 1) * sizeof(ppp_registration_row), hipMemcpyDeviceToHost));
    if (!C.done) { /* the evaluation behind the last step: no step kernel follows it */
        unsigned long long acc[ICP_WORDS];
        double Tl[12];
        HIPCHK(h, copy_sync(h, acc, G.acc.p + ICP_WORDS * last, sizeof(acc), hipMemcpyDeviceToHost));
        HIPCHK(h, copy_sync(h, Tl, G.T.p + 12 * last, sizeof(Tl), hipMemcpyDeviceToHost));
        icp_row_terms(&R[last], Tl, acc);
    }
    if (R[0].pairs > (size_t)std::max(nq, 0) || R[last].pairs > (size_t)std::max(nq, 0)) return fail(h, PPP_ERR_HIP, std::string(w) + ": sums corrupt");
    return PPP_OK;
}

/* The registration chain: the reference's index and normal field on its own stream, one wait for that stream,
   then iterations + 1 evaluations (k_reg_terms) and iterations steps (k_reg_step) back to back on the scan's stream -- the
   transforms, the sums and the rows stay on the device, a chain that has ended turns the rest of its launches into returns --
   and one wait.  !loop: the one evaluation of ppp_get_registration_terms.  trim (ppp_register_trimmed): an
   evaluation is k_trim_pair, k_trim_narrow<1>, k_trim_narrow<2> and k_trim_terms instead of k_reg_terms -- its 29 words are over
   the kept pairs --, k_trim_scatter follows the chain, and the rows and the maps go to trim's arrays. */
struct TrimCall {
    double keep;
    ppp_trimmed_registration_row *rows;
    unsigned char *status;
    float *d2;
    size_t cap;
};

static int registration_chain(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T0, bool loop,
                              ppp_registration_row *rows, size_t row_cap, ppp_registration_stats *stats, const TrimCall *trim = nullptr)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!ref || !rp) return fail(h, PPP_ERR_ARG, "registration: no reference handle or no parameters");
    if (!rows && !(trim && trim->rows) && row_cap) return fail(h, PPP_ERR_ARG, "registration: rows is NULL with row_cap > 0");
    if (trim && !(trim->keep > 0.0 && trim->keep <= 1.0)) return fail(h, PPP_ERR_ARG, "trimmed registration: keep must be in (0, 1]");
    const ppp_registration_params P = *rp;
    IcpFrame F;
    int rc = registration_params_ok(h, P, F);
    if (rc) return rc;
    const int iterations = loop ? P.iterations : 0;
    double T[12];
    rc = opening_transform(h, "registration", T0, T);
    if (rc) return rc;
    int shift = 0;
    rc = registration_setup(h, ref, P, F, shift);
    if (rc) return rc;
    const size_t N = h->n;
    const int nq = h->hmeta.n_sorted, nref = ref->hmeta.n_sorted;
    auto &G = h->registration;
    const size_t evals = (size_t)iterations + 1;
    rc = chain_open(h, evals, T);
    if (rc) return rc;
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.ctl.p);
    /* grid-stride: the workgroups, and with them the atomics of an evaluation, are capped by the device, not by the cloud */
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)nq + ICP_T - 1) / ICP_T, 2 * (size_t)h->num_cus));
    const size_t N1 = std::max<size_t>(N, 1);
    TrimCut *cuts = nullptr;
    if (trim) {
        static_assert(sizeof(TrimCut) == 8 * sizeof(unsigned), "TrimCut is eight words");
        HIPCHK(h, G.partner.ensure(std::max<size_t>((size_t)std::max(nq, 0), 1))); HIPCHK(h, G.key.ensure(std::max<size_t>((size_t)std::max(nq, 0), 1)));
        HIPCHK(h, G.hist.ensure(TRIM_WORDS * evals)); HIPCHK(h, G.cuts.ensure(8 * evals));
        HIPCHK(h, G.tstatus.ensure(N1)); HIPCHK(h, G.td2.ensure(N1));
        cuts = reinterpret_cast<TrimCut *>(G.cuts.p);
        /* every evaluation has histograms of its own: one clear on the stream before the chain, none between iterations */
        HIPCHK(h, hipMemsetAsync(G.hist.p, 0, TRIM_WORDS * evals * sizeof(unsigned), h->stream));
        HIPCHK(h, hipMemsetAsync(G.cuts.p, 0, 8 * evals * sizeof(unsigned), h->stream));
        HIPCHK(h, hipMemsetAsync(G.tstatus.p, PPP_TRIM_DROPPED, N1, h->stream)); /* points outside the index: not finite */
        HIPCHK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(G.td2.p), (int)TRIM_NAN, N1, h->stream));
    }
    for (int k = 0; k <= iterations; ++k) {
        if (trim) {
            unsigned *hist = G.hist.p + TRIM_WORDS * (size_t)k;
            LAUNCH(h, "k_trim_pair", k_trim_pair, grid, TRIM_T, 0, h->sorted4.p, nq, contact_index(ref), nref, F, G.T.p + 12 * (size_t)k, ctl,
                   G.partner.p, G.key.p, hist);
            LAUNCH(h, "k_trim_narrow<1>", k_trim_narrow<1>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist, hist + TRIM_B0, trim->keep, cuts + k);
            LAUNCH(h, "k_trim_narrow<2>", k_trim_narrow<2>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist + TRIM_B0, hist + TRIM_B0 + TRIM_B1, trim->keep,
                   cuts + k);
            LAUNCH(h, "k_trim_terms", k_trim_terms, grid, TRIM_T, 0, h->sorted4.p, nq, contact_index(ref), F, G.T.p + 12 * (size_t)k, ctl, G.partner.p,
                   G.key.p, hist + TRIM_B0 + TRIM_B1, cuts + k, G.acc.p + ICP_WORDS * (size_t)k);
        } else
            LAUNCH(h, "k_reg_terms", k_reg_terms, grid, ICP_T, 0, h->sorted4.p, nq, contact_index(ref), nref, F, G.T.p + 12 * (size_t)k, ctl,
                   G.acc.p + ICP_WORDS * (size_t)k);
        if (k < iterations)
            LAUNCH(h, "k_reg_step", k_reg_step, 1, 64, 0, G.acc.p + ICP_WORDS * (size_t)k, F, G.T.p + 12 * (size_t)k, G.rows.p + k, ctl);
    }
    if (trim)
        LAUNCH(h, "k_trim_scatter", k_trim_scatter, grid, TRIM_T, 0, h->sorted4.p, nq, G.key.p, ctl, cuts, (int)evals, (int)N1, G.tstatus.p, G.td2.p);
    IcpCtl C;
    std::vector<ppp_registration_row> R;
    rc = chain_collect(h, "registration", iterations, nq, C, R);
    if (rc) return rc;
    const size_t last = (size_t)C.steps;
    if (stats) *stats = registration_stats(R, C, N, (size_t)nq, shift, F.c, F.Ln);
    const size_t k = std::min(row_cap, last + 1);
    if (rows && k) memcpy(rows, R.data(), k * sizeof(ppp_registration_row));
    if (trim) {
        std::vector<TrimCut> cut(last + 1);
        HIPCHK(h, copy_sync(h, cut.data(), G.cuts.p, (last + 1) * sizeof(TrimCut), hipMemcpyDeviceToHost));
        for (size_t i = 0; i <= last; ++i)
            if (cut[i].paired > (unsigned)std::max(nq, 0) || R[i].pairs > cut[i].paired || (cut[i].paired && R[i].pairs < cut[i].k))
                return fail(h, PPP_ERR_HIP, "trimmed registration: cut corrupt");
        for (size_t i = 0; trim->rows && i < k; ++i) trimmed_row(trim->rows[i], R[i], cut[i].paired, cut[i].tau);
        const size_t m = std::min(trim->cap, N);
        if (trim->status && m) HIPCHK(h, copy_sync(h, trim->status, G.tstatus.p, m, hipMemcpyDeviceToHost));
        if (trim->d2 && m) HIPCHK(h, copy_sync(h, trim->d2, G.td2.p, m * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PPP_OK;
}

int ppp_get_registration_terms(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T12, ppp_registration_row *row,
                               ppp_registration_stats *stats)
{
    return registration_chain(h, ref, rp, T12, false, row, row ? 1 : 0, stats);
}

int ppp_register(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T0_12, ppp_registration_row *rows, size_t row_cap,
                 ppp_registration_stats *stats)
{
    return registration_chain(h, ref, rp, T0_12, true, rows, row_cap, stats);
}

void ppp_default_trimmed_registration_params(ppp_trimmed_registration_params *tp)
{
    if (!tp) return;
    ppp_default_registration_params(&tp->icp);
    tp->keep = 0.8;
}

int ppp_register_trimmed(ppp_handle h, ppp_handle ref, const ppp_trimmed_registration_params *tp, const double *T0_12,
                         ppp_trimmed_registration_row *rows, size_t row_cap, unsigned char *status, float *d2, size_t cap,
                         ppp_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    if (!tp) return fail(h, PPP_ERR_ARG, "trimmed registration: no parameters");
    const TrimCall trim = {tp->keep, rows, status, d2, cap};
    return registration_chain(h, ref, &tp->icp, T0_12, true, nullptr, row_cap, stats, &trim);
}

void ppp_default_robust_registration_params(ppp_robust_registration_params *bp)
{
    if (!bp) return;
    ppp_default_registration_params(&bp->icp);
    bp->tune = 4.685; bp->sigma_min = 1e-4;
}

/* What ppp_register_robust's chain and ppp_register_mesh_robust's have in common on either side of their launches, as chain_open
   and chain_collect are for the unweighted pair.  robust_open: room for `evals` evaluations of ROB_WORDS words, their histograms,
   cuts and sigmas, the per-query keys and residuals and the three maps in h->registration's buffers; the words, the control
   block, the histograms, the cuts and the sigmas cleared on h's stream (every evaluation has histograms of its own: one clear
   before the chain, none between iterations); T at the chain's head; k_rob_fill over the maps.  robust_collect: the one wait, the
   sanity checks (w: the call's name), then the rows, the statistics and the maps as ppp_register_robust hands them out. */
static int robust_open(ppp_handle h, size_t evals, int nq, const double *T)
{
    auto &G = h->registration;
    const size_t N1 = std::max<size_t>(h->n, 1), nq1 = std::max<size_t>((size_t)std::max(nq, 0), 1);
    static_assert(sizeof(TrimCut) == 8 * sizeof(unsigned), "TrimCut is eight words");
    HIPCHK(h, G.T.ensure(12 * evals)); HIPCHK(h, G.acc.ensure(ROB_WORDS * evals)); HIPCHK(h, G.rows.ensure(evals)); HIPCHK(h, G.ctl.ensure(8));
    HIPCHK(h, G.key.ensure(nq1)); HIPCHK(h, G.rres.ensure(nq1));
    HIPCHK(h, G.hist.ensure(TRIM_WORDS * evals)); HIPCHK(h, G.cuts.ensure(8 * evals)); HIPCHK(h, G.rsigma.ensure(evals));
    HIPCHK(h, G.tstatus.ensure(N1)); HIPCHK(h, G.td2.ensure(N1)); HIPCHK(h, G.rresid.ensure(N1));
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, ROB_WORDS * evals * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(G.ctl.p, 0, 8 * sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(G.hist.p, 0, TRIM_WORDS * evals * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(G.cuts.p, 0, 8 * evals * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(G.rsigma.p, 0, evals * sizeof(double), h->stream));
    HIPCHK(h, copy_sync(h, G.T.p, T, 12 * sizeof(double), hipMemcpyHostToDevice));
    LAUNCH(h, "k_rob_fill", k_rob_fill, (unsigned)std::min<size_t>((N1 + TRIM_T - 1) / TRIM_T, 2 * (size_t)h->num_cus), TRIM_T, 0, (int)N1, G.tstatus.p,
           G.td2.p, G.rresid.p); /* points outside the index: not finite */
    return PPP_OK;
}

static int robust_collect(ppp_handle h, const char *w, int iterations, int nq, int shift, const IcpFrame &F, ppp_robust_registration_row *rows,
                          size_t row_cap, unsigned char *status, float *weight, double *residual, size_t cap, ppp_registration_stats *stats)
{
    auto &G = h->registration;
    const size_t N = h->n;
    IcpCtl C;
    HIPCHK(h, copy_sync(h, &C, G.ctl.p, sizeof(C), hipMemcpyDeviceToHost)); /* the one wait */
    if (!chain_ctl_ok(C, iterations)) return fail(h, PPP_ERR_HIP, std::string(w) + ": control words corrupt");
    const size_t last = (size_t)C.steps;
    std::vector<ppp_registration_row> R(last + 1);
    std::vector<unsigned long long> acc(ROB_WORDS * (last + 1));
    std::vector<TrimCut> cut(last + 1);
    std::vector<double> sigma(last + 1);
    HIPCHK(h, copy_sync(h, R.data(), G.rows.p, (last + 1) * sizeof(ppp_registration_row), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, acc.data(), G.acc.p, acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, cut.data(), G.cuts.p, (last + 1) * sizeof(TrimCut), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, sigma.data(), G.rsigma.p, (last + 1) * sizeof(double), hipMemcpyDeviceToHost));
    if (!C.done) { /* the evaluation behind the last step: no step kernel follows it */
        double Tl[12];
        HIPCHK(h, copy_sync(h, Tl, G.T.p + 12 * last, sizeof(Tl), hipMemcpyDeviceToHost));
        icp_row_terms(&R[last], Tl, acc.data() + ROB_WORDS * last);
    }
    std::vector<ppp_robust_registration_row> out(last + 1);
    for (size_t i = 0; i <= last; ++i) {
        const unsigned long long *a = acc.data() + ROB_WORDS * i;
        if (cut[i].paired > (unsigned)std::max(nq, 0) || a[ROB_USED] > cut[i].paired || R[i].pairs != (size_t)a[ROB_USED])
            return fail(h, PPP_ERR_HIP, std::string(w) + ": sums corrupt");
        ppp_robust_registration_row &o = out[i];
        memset(&o, 0, sizeof(o)); /* the padding too: rows compare as bytes */
        o.row = R[i];
        o.row.pairs = cut[i].paired; /* the step kernel read `used` there */
        o.used = (size_t)a[ROB_USED];
        o.weight_sum = (long long)a[ROB_WSUM];
        memcpy(&o.median_abs, &cut[i].tau, sizeof(float));
        o.sigma = sigma[i];
        R[i].pairs = cut[i].paired;
    }
    if (stats) {
        *stats = registration_stats(R, C, N, (size_t)nq, shift, F.c, F.Ln);
        auto rms = [](const ppp_robust_registration_row &r) { return r.weight_sum ? std::sqrt((double)r.row.E / (double)r.weight_sum) : (double)NAN; };
        stats->rms_before = rms(out[0]); stats->rms_after = rms(out[last]);
    }
    const size_t k = std::min(row_cap, last + 1);
    if (rows && k) memcpy(rows, out.data(), k * sizeof(ppp_robust_registration_row));
    const size_t m = std::min(cap, N);
    if (status && m) HIPCHK(h, copy_sync(h, status, G.tstatus.p, m, hipMemcpyDeviceToHost));
    if (weight && m) HIPCHK(h, copy_sync(h, weight, G.td2.p, m * sizeof(float), hipMemcpyDeviceToHost));
    if (residual && m) HIPCHK(h, copy_sync(h, residual, G.rresid.p, m * sizeof(double), hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* the two parameters a robust chain has beside ppp_register's, checked (w: the call's name) */
static int robust_params_ok(ppp_handle h, const char *w, const ppp_robust_registration_params *bp)
{
    if (!(bp->tune > 0.0)) return fail(h, PPP_ERR_ARG, std::string(w) + ": tune must be > 0 (+INFINITY: every weight is 1)");
    if (!(bp->sigma_min >= 0.0 && std::isfinite(bp->sigma_min))) return fail(h, PPP_ERR_ARG, std::string(w) + ": sigma_min must be finite and >= 0");
    return PPP_OK;
}

/* The robust chain: registration_chain's shape -- the reference's index and normal field on its own stream, one
   wait for that stream, then iterations + 1 evaluations and iterations steps back to back on the scan's stream, and one wait --
   in which an evaluation is k_rob_pair, k_trim_narrow<1>, k_trim_narrow<2> at keep 0.5 and k_rob_terms, its ROB_WORDS words
   the weighted sums with `used` in word 0, which is what k_reg_step reads as its pairs; k_rob_scatter follows the chain.
   !loop: the one evaluation of ppp_get_robust_registration_terms. */
static int robust_chain(ppp_handle h, ppp_handle ref, const ppp_robust_registration_params *bp, const double *T0, bool loop,
                        ppp_robust_registration_row *rows, size_t row_cap, unsigned char *status, float *weight, double *residual, size_t cap,
                        ppp_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!ref || !bp) return fail(h, PPP_ERR_ARG, "robust registration: no reference handle or no parameters");
    if (!rows && row_cap) return fail(h, PPP_ERR_ARG, "robust registration: rows is NULL with row_cap > 0");
    int rc = robust_params_ok(h, "robust registration", bp);
    if (rc) return rc;
    const ppp_registration_params P = bp->icp;
    const RobScale S = {bp->tune, bp->sigma_min};
    IcpFrame F;
    rc = registration_params_ok(h, P, F);
    if (rc) return rc;
    const int iterations = loop ? P.iterations : 0;
    double T[12];
    rc = opening_transform(h, "robust registration", T0, T);
    if (rc) return rc;
    int shift = 0;
    rc = registration_setup(h, ref, P, F, shift);
    if (rc) return rc;
    const int nq = h->hmeta.n_sorted, nref = ref->hmeta.n_sorted;
    auto &G = h->registration;
    const size_t evals = (size_t)iterations + 1;
    HIPCHK(h, G.partner.ensure(std::max<size_t>((size_t)std::max(nq, 0), 1)));
    rc = robust_open(h, evals, nq, T);
    if (rc) return rc;
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.ctl.p);
    TrimCut *cuts = reinterpret_cast<TrimCut *>(G.cuts.p);
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)nq + TRIM_T - 1) / TRIM_T, 2 * (size_t)h->num_cus));
    for (int k = 0; k <= iterations; ++k) {
        unsigned *hist = G.hist.p + TRIM_WORDS * (size_t)k;
        unsigned long long *acc = G.acc.p + ROB_WORDS * (size_t)k;
        LAUNCH(h, "k_rob_pair", k_rob_pair, grid, TRIM_T, 0, h->sorted4.p, nq, contact_index(ref), nref, F, G.T.p + 12 * (size_t)k, ctl, G.partner.p,
               G.rres.p, G.key.p, hist);
        LAUNCH(h, "k_trim_narrow<1>", k_trim_narrow<1>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist, hist + TRIM_B0, ROB_KEEP, cuts + k);
        LAUNCH(h, "k_trim_narrow<2>", k_trim_narrow<2>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist + TRIM_B0, hist + TRIM_B0 + TRIM_B1, ROB_KEEP, cuts + k);
        LAUNCH(h, "k_rob_terms", k_rob_terms, grid, TRIM_T, 0, h->sorted4.p, nq, contact_index(ref), F, S, G.T.p + 12 * (size_t)k, ctl, G.partner.p,
               G.rres.p, G.key.p, hist + TRIM_B0 + TRIM_B1, cuts + k, G.rsigma.p + k, acc);
        if (k < iterations) LAUNCH(h, "k_reg_step", k_reg_step, 1, 64, 0, acc, F, G.T.p + 12 * (size_t)k, G.rows.p + k, ctl);
    }
    LAUNCH(h, "k_rob_scatter", k_rob_scatter, grid, TRIM_T, 0, h->sorted4.p, nq, G.key.p, G.rres.p, ctl, cuts, G.rsigma.p, S, (int)evals,
           (int)std::max<size_t>(h->n, 1), G.tstatus.p, G.td2.p, G.rresid.p);
    return robust_collect(h, "robust registration", iterations, nq, shift, F, rows, row_cap, status, weight, residual, cap, stats);
}

int ppp_get_robust_registration_terms(ppp_handle h, ppp_handle ref, const ppp_robust_registration_params *bp, const double *T12,
                                      ppp_robust_registration_row *row, unsigned char *status, float *weight, double *residual, size_t cap,
                                      ppp_registration_stats *stats)
{
    return robust_chain(h, ref, bp, T12, false, row, row ? 1 : 0, status, weight, residual, cap, stats);
}

int ppp_register_robust(ppp_handle h, ppp_handle ref, const ppp_robust_registration_params *bp, const double *T0_12,
                        ppp_robust_registration_row *rows, size_t row_cap, unsigned char *status, float *weight, double *residual, size_t cap,
                        ppp_registration_stats *stats)
{
    return robust_chain(h, ref, bp, T0_12, true, rows, row_cap, status, weight, residual, cap, stats);
}

/* The ten words of side's cloud (k_cloud_moments on side's stream, one wait) and the frame they imply; side's index is
   complete (deviation_side).  Errors are reported on h. */
static int cloud_moments(ppp_handle h, ppp_handle side, const char *who, ppp_cloud_frame *frame)
{
    const std::string w = std::string("cloud moments: ") + who;
    auto run = [&]() -> int {
        int rc = fetch_meta(side);
        if (rc) return rc;
        const int nq = side->hmeta.n_sorted;
        if (nq <= 0) return fail(side, PPP_ERR_ARG, "no indexed point");
        MomFrame F;
        const int ms = mom_shift(side->n);
        frame_from_bounds(side->hmeta.mn, side->hmeta.mx, 0.0, ms, F.c, &F.L, &F.scale); /* (+ 0.0 changes no bit of an extent) */
        if (!(F.L > 0.0 && std::isfinite(F.L))) return fail(side, PPP_ERR_ARG, "the box of the cloud has no extent (L == 0)");
        auto &G = side->registration;
        HIPCHK(side, G.mom.ensure(MOM_WORDS));
        HIPCHK(side, hipMemsetAsync(G.mom.p, 0, MOM_WORDS * sizeof(unsigned long long), side->stream));
        const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)nq + MOM_T - 1) / MOM_T, 2 * (size_t)side->num_cus));
        LAUNCH(side, "k_cloud_moments", k_cloud_moments, grid, MOM_T, 0, side->sorted4.p, nq, F, G.mom.p);
        unsigned long long acc[MOM_WORDS];
        HIPCHK(side, copy_sync(side, acc, G.mom.p, sizeof(acc), hipMemcpyDeviceToHost));
        long long words[MOM_WORDS];
        for (int i = 0; i < MOM_WORDS; ++i) words[i] = (long long)acc[i];
        if (words[0] != (long long)nq) return fail(side, PPP_ERR_HIP, "sums corrupt");
        if (!cloud_frame_from_words(words, ms, F.c, F.L, frame)) return fail(side, PPP_ERR_HIP, "sums corrupt");
        return PPP_OK;
    };
    const int rc = run();
    return rc ? fail(h, rc, w + ": " + side->err) : PPP_OK;
}

int ppp_get_cloud_moments(ppp_handle h, ppp_cloud_frame *frame)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!frame) return fail(h, PPP_ERR_ARG, "cloud moments: frame is NULL");
    int rc = deviation_side(h, h, "the cloud", "cloud moments");
    if (rc) return rc;
    return cloud_moments(h, h, "the cloud", frame);
}

int ppp_cloud_frame_from_moments(const long long *words10, int ms, const double *c3, double L, ppp_cloud_frame *frame)
{
    if (!words10 || !c3 || !frame) return PPP_ERR_ARG;
    return cloud_frame_from_words(words10, ms, c3, L, frame) ? PPP_OK : PPP_ERR_ARG;
}

int ppp_registration_starts(const ppp_cloud_frame *scan, const ppp_cloud_frame *ref, int candidates, double *T12s)
{
    if (!scan || !ref || !T12s || (candidates != 4 && candidates != 24)) return PPP_ERR_ARG;
    registration_starts(scan, ref, candidates, T12s);
    return PPP_OK;
}

void ppp_default_global_registration_params(ppp_global_registration_params *gp)
{
    if (!gp) return;
    gp->candidates = 24; gp->stride = 16;
    gp->coarse.max_dist = 10.f; gp->coarse.iterations = 8; gp->coarse.min_step = 1e-3; gp->coarse.lock_eps = 1e-9;
    ppp_default_registration_params(&gp->fine);
}

/* What ppp_register_global and ppp_register_mesh_global have in common on either side of their coarse launches (w: the call's
   name).  global_params_ok: the refusals for the caller's arrays and for gp; F and Ffine take what the two parameter sets set.
   coarse_open: the starts the two frames imply (B.75), room for K chains in h->registration's buffers, the queries compacted
   once (StrideSel), the words and the control blocks cleared on h's stream, every chain's start at its head.  coarse_collect: the
   one wait, the sanity checks, the candidate table with B.76's cost, the winner and second_cost.  global_results: the
   statistics behind the fine chain and the caller's share of the table. */
struct CoarseStage {
    int K = 0, iterations = 0, nq = 0;
    size_t evals = 0, tstride = 0, astride = 0;
    std::vector<double> T, T0;
    IcpCtl *ctl = nullptr;
    std::vector<ppp_registration_candidate> cands;
    int winner = 0;
    long long second = -1;
};

static int global_params_ok(ppp_handle h, const std::string &w, const ppp_global_registration_params &P, const void *cands, size_t cand_cap,
                            const void *rows, size_t row_cap, IcpFrame &F, IcpFrame &Ffine)
{
    if (!rows && row_cap) return fail(h, PPP_ERR_ARG, w + ": rows is NULL with row_cap > 0");
    if (!cands && cand_cap) return fail(h, PPP_ERR_ARG, w + ": cands is NULL with cand_cap > 0");
    if (P.candidates != 4 && P.candidates != 24) return fail(h, PPP_ERR_ARG, w + ": candidates must be 4 or 24");
    if (P.stride < 1) return fail(h, PPP_ERR_ARG, w + ": stride must be >= 1");
    const int rc = registration_params_ok(h, P.coarse, F);
    return rc ? rc : registration_params_ok(h, P.fine, Ffine);
}

static int coarse_open(ppp_handle h, const std::string &w, const ppp_global_registration_params &P, const ppp_cloud_frame &scan, const ppp_cloud_frame &ref,
                       CoarseStage &S)
{
    const int K = S.K = P.candidates;
    S.iterations = P.coarse.iterations;
    const size_t evals = S.evals = (size_t)S.iterations + 1;
    S.tstride = 12 * evals; S.astride = ICP_WORDS * evals;
    S.T.assign((size_t)K * evals * 12, 0.0); S.T0.resize((size_t)K * 12);
    registration_starts(&scan, &ref, K, S.T0.data());
    for (double v : S.T0) if (!std::isfinite(v)) return fail(h, PPP_ERR_ARG, w + ": a start has an entry that is not finite");
    for (int s = 0; s < K; ++s) memcpy(&S.T[(size_t)s * evals * 12], &S.T0[(size_t)s * 12], 12 * sizeof(double));
    const int ns = h->hmeta.n_sorted;
    auto &G = h->registration;
    const size_t ns1 = (size_t)std::max(ns, 1);
    HIPCHK(h, G.queries.ensure(ns1)); HIPCHK(h, G.qcnt.ensure((ns1 + COMPACT_CHUNK - 1) / COMPACT_CHUNK + 1));
    HIPCHK(h, G.mT.ensure(S.T.size())); HIPCHK(h, G.macc.ensure(ICP_WORDS * evals * K)); HIPCHK(h, G.mrows.ensure(evals * K)); HIPCHK(h, G.mctl.ensure(5 * (size_t)K));
    int nq = 0;
    if (ns > 0) {
        const int nblocks = (ns + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
        StrideSel sel = {h->sorted4.p, P.stride, G.queries.p};
        const int rc = compact(h, sel, ns, G.qcnt.p, G.qcnt.p + nblocks, [&](int kept) -> int {
            if (kept < 0 || kept > ns) return fail(h, PPP_ERR_HIP, w + ": query count corrupt");
            nq = kept;
            return PPP_OK;
        });
        if (rc) return rc;
    }
    if (nq <= 0) return fail(h, PPP_ERR_ARG, w + ": no query left (no indexed point has a cloud index that is a multiple of stride)");
    S.nq = nq;
    HIPCHK(h, hipMemsetAsync(G.macc.p, 0, ICP_WORDS * evals * K * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(G.mctl.p, 0, 5 * (size_t)K * sizeof(int), h->stream));
    HIPCHK(h, copy_sync(h, G.mT.p, S.T.data(), S.T.size() * sizeof(double), hipMemcpyHostToDevice));
    S.ctl = reinterpret_cast<IcpCtl *>(G.mctl.p);
    return PPP_OK;
}

static int coarse_collect(ppp_handle h, const std::string &w, const IcpFrame &F, CoarseStage &S)
{
    const int K = S.K, nq = S.nq;
    const size_t evals = S.evals;
    auto &G = h->registration;
    std::vector<IcpCtl> C((size_t)K);
    std::vector<ppp_registration_row> R(evals * K);
    std::vector<unsigned long long> acc(ICP_WORDS * evals * K);
    HIPCHK(h, copy_sync(h, C.data(), G.mctl.p, C.size() * sizeof(IcpCtl), hipMemcpyDeviceToHost)); /* the one wait */
    HIPCHK(h, copy_sync(h, R.data(), G.mrows.p, R.size() * sizeof(ppp_registration_row), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, acc.data(), G.macc.p, acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, S.T.data(), G.mT.p, S.T.size() * sizeof(double), hipMemcpyDeviceToHost));
    const long long far = llrint((double)F.md2 * F.scale);
    std::vector<ppp_registration_candidate> &cd = S.cands;
    cd.assign((size_t)K, ppp_registration_candidate{});
    int win = 0;
    for (int s = 0; s < K; ++s) {
        const IcpCtl &c = C[(size_t)s];
        if (!chain_ctl_ok(c, S.iterations)) return fail(h, PPP_ERR_HIP, w + ": control words corrupt");
        const size_t first = (size_t)s * evals, last = first + (size_t)c.steps;
        if (!c.done) icp_row_terms(&R[last], &S.T[12 * last], &acc[ICP_WORDS * last]); /* the evaluation behind the last step: no step kernel follows it */
        if (R[first].pairs > (size_t)nq || R[last].pairs > (size_t)nq) return fail(h, PPP_ERR_HIP, w + ": sums corrupt");
        ppp_registration_candidate &o = cd[(size_t)s];
        o.index = s;
        memcpy(o.T0, &S.T0[12 * (size_t)s], sizeof(o.T0)); memcpy(o.T, R[last].T, sizeof(o.T));
        o.steps = c.steps; o.converged = c.converged; o.locked = c.locked;
        o.pairs0 = R[first].pairs; o.E0 = R[first].E; o.pairs = R[last].pairs; o.E = R[last].E;
        o.cost = o.E + (long long)((size_t)nq - o.pairs) * far;
        if (o.cost < cd[(size_t)win].cost) win = s;
    }
    long long second = -1;
    for (int s = 0; s < K; ++s)
        if (memcmp(cd[(size_t)s].T, cd[(size_t)win].T, sizeof(cd[0].T)) != 0 && (second < 0 || cd[(size_t)s].cost < second)) second = cd[(size_t)s].cost;
    S.winner = win; S.second = second;
    return PPP_OK;
}

static void global_results(const CoarseStage &S, int shift, ppp_global_registration_stats &st, ppp_global_registration_stats *stats,
                           ppp_registration_candidate *cands, size_t cand_cap)
{
    st.queries = (size_t)S.nq; st.shift = shift; st.candidates = S.K; st.winner = S.winner;
    st.winner_cost = S.cands[(size_t)S.winner].cost; st.second_cost = S.second;
    if (stats) *stats = st;
    const size_t k = std::min(cand_cap, (size_t)S.K);
    if (cands && k) memcpy(cands, S.cands.data(), k * sizeof(ppp_registration_candidate));
}

/* Global registration: both clouds' moments, the starts their frames imply, then every start's coarse chain
   side by side -- coarse.iterations + 1 launches of k_reg_terms_multi and coarse.iterations of k_reg_step_multi back to back
   on h's stream, on the queries compacted once -- one wait, the winner by cost on the host, and registration_chain from it. */
int ppp_register_global(ppp_handle h, ppp_handle ref, const ppp_global_registration_params *gp, ppp_registration_candidate *cands, size_t cand_cap,
                        ppp_registration_row *rows, size_t row_cap, ppp_global_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!ref || !gp) return fail(h, PPP_ERR_ARG, "global registration: no reference handle or no parameters");
    const ppp_global_registration_params P = *gp;
    IcpFrame F, Ffine;
    int rc = global_params_ok(h, "global registration", P, cands, cand_cap, rows, row_cap, F, Ffine);
    if (rc) return rc;
    int shift = 0;
    rc = registration_setup(h, ref, P.coarse, F, shift);
    if (rc) return rc;
    if (icp_shift(h->n, Ffine.md2) < 16)
        return fail(h, PPP_ERR_ARG, "registration: fewer than 16 fractional bits are left (n max_dist^2 too large): the integer sums could overflow");
    ppp_global_registration_stats st = {};
    rc = cloud_moments(h, h, "the scan", &st.scan);
    if (rc) return rc;
    if (ref == h) st.ref = st.scan;
    else { rc = cloud_moments(h, ref, "the reference", &st.ref); if (rc) return rc; }
    CoarseStage S;
    rc = coarse_open(h, "global registration", P, st.scan, st.ref, S);
    if (rc) return rc;
    const int K = S.K, nq = S.nq, nref = ref->hmeta.n_sorted;
    auto &G = h->registration;
    /* all starts together stay at two workgroups per CU, and never below one per start */
    const size_t per = std::max<size_t>(1, std::min<size_t>(((size_t)nq + ICP_T - 1) / ICP_T, 2 * (size_t)h->num_cus / (size_t)K));
    for (int k = 0; k <= S.iterations; ++k) {
        LAUNCH(h, "k_reg_terms_multi", k_reg_terms_multi, dim3((unsigned)per, (unsigned)K), ICP_T, 0, G.queries.p, nq, contact_index(ref), nref, F,
               G.mT.p + 12 * (size_t)k, S.tstride, S.ctl, G.macc.p + ICP_WORDS * (size_t)k, S.astride);
        if (k < S.iterations)
            LAUNCH(h, "k_reg_step_multi", k_reg_step_multi, K, 64, 0, G.macc.p + ICP_WORDS * (size_t)k, S.astride, F, G.mT.p + 12 * (size_t)k, S.tstride,
                   G.mrows.p + k, S.evals, S.ctl);
    }
    rc = coarse_collect(h, "global registration", F, S);
    if (rc) return rc;
    rc = registration_chain(h, ref, &P.fine, S.cands[(size_t)S.winner].T, true, rows, row_cap, &st.fine);
    if (rc) return rc;
    global_results(S, shift, st, stats, cands, cand_cap);
    return PPP_OK;
}

/* [own_lo, own_hi) widened by r with room for the roundings (B.82): r times the 1.0001 of the margin tests, which covers the
   float product dx dx against r r, and one float further out, which covers the rounding of the sum itself -- at coordinates of
   metres half an ulp is more than r / 10 000.  An empty interval stays empty. */
static void widened(const TileRange &T, float r, float &lo, float &hi)
{
    lo = nextafterf(T.own_lo - r * 1.0001f, -INFINITY); hi = nextafterf(T.own_hi + r * 1.0001f, INFINITY);
}

/* the slabs [b0, b1) a handle's index sorted: all of them, or those of a slice-range handle's interval (slab_geom) */
static void sorted_slabs(const ppp_handle s, int &b0, int &b1)
{
    const SlabGeom G = slab_geom(s);
    b0 = G.first_slab; b1 = std::min(s->B, G.first_slab + G.g_sort);
}

/* The deviation map of the points h owns: both plans, the range checks on the host, both indices, then the
   reference's normal field on its own stream, one wait for that stream, k_devt_fill, k_devt_nearest, k_devt_smooth where asked and
   k_devt_target back to back on the scan's stream, and one wait.  The buffers are ppp_get_deviation's: nothing is kept. */
int ppp_get_deviation_tile(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp, float halo, double *deviation, double *smoothed,
                           int *ref_index, unsigned char *status, double *target, unsigned char *owned, size_t cap,
                           ppp_deviation_tile_stats *part)
{
    int rc = deviation_call_ok(h, ref, dp, "deviation tile", &halo);
    if (rc) return rc;
    const ppp_deviation_params P = *dp;
    const bool smooth = P.smooth_radius > 0.f;
    rc = deviation_side_cloud(h, ref, "deviation tile: the reference", true);
    if (rc) return rc;
    if (ref != h) { rc = deviation_side_cloud(h, h, "deviation tile: the scan", true); if (rc) return rc; }
    const size_t N = h->n;
    if (deviation_sum_overflows(P, N)) return fail(h, PPP_ERR_ARG, "deviation tile: max_dist 2^24 n reaches 2^62: the smoothing's integer sum could overflow");
    /* From the two plans alone, before an index is built or a kernel launched.  What is evaluated: the owned interval widened by
       smooth_radius.  What the reference must index: the owned interval widened by halo, and by its normal_radius beyond that --
       the normal of a partner at the halo's edge reads that neighbourhood. */
    TileRange T;
    rc = tile_range(h, 0.f, T);
    if (rc) return rc;
    widened(T, P.smooth_radius, T.ev_lo, T.ev_hi);
    if (leaves_indexed_range(h, T.ev_lo, T.ev_hi))
        return fail(h, PPP_ERR_ARG, "deviation tile: the owned interval widened by smooth_radius reaches beyond the scan's indexed slice range: raise range_margin");
    float need_lo, need_hi;
    widened(T, halo + ref->P.normal_radius, need_lo, need_hi);
    if (leaves_indexed_range(ref, need_lo, need_hi))
        return fail(h, PPP_ERR_ARG, "deviation tile: the reference's indexed slice range does not cover the owned interval widened by halo + normal_radius");
    rc = deviation_side_index(h, ref, "deviation tile: the reference", false);
    if (rc) return rc;
    if (ref != h) { rc = deviation_side_index(h, h, "deviation tile: the scan", false); if (rc) return rc; }
    rc = reference_normals(h, ref, "deviation tile");
    if (rc) return rc;
    int pos0, pos1, hb0, hb1, rb0, rb1;
    rc = tile_positions(h, T, pos0, pos1);
    if (rc) return rc;
    sorted_slabs(h, hb0, hb1); sorted_slabs(ref, rb0, rb1);
    auto &D = h->deviation;
    const size_t N1 = std::max<size_t>(N, 1);
    HIPCHK(h, D.dev.ensure(N1)); HIPCHK(h, D.target.ensure(N1)); HIPCHK(h, D.fix.ensure(N1)); HIPCHK(h, D.d2.ensure(N1));
    HIPCHK(h, D.ref_index.ensure(N1)); HIPCHK(h, D.status.ensure(N1)); HIPCHK(h, D.owned.ensure(N1)); HIPCHK(h, D.acc.ensure(DEV_ACC_WORDS));
    if (smooth) HIPCHK(h, D.smoothed.ensure(N1));
    double *v = smooth ? D.smoothed.p : D.dev.p;
    HIPCHK(h, hipMemsetAsync(D.acc.p, 0, DEVT_ACC_WORDS * sizeof(unsigned long long), h->stream));
    const size_t cap_grid = 2 * (size_t)h->num_cus;
    LAUNCH(h, "k_devt_fill", k_devt_fill, (unsigned)std::min<size_t>((N1 + DEV_T - 1) / DEV_T, cap_grid), DEV_T, 0, (int)N, D.dev.p,
           smooth ? D.smoothed.p : nullptr, D.target.p, D.ref_index.p, D.status.p, D.owned.p);
    if (pos1 > pos0) {
        const size_t gq = ((size_t)(pos1 - pos0) + DEV_T - 1) / DEV_T;
        LAUNCH(h, "k_devt_nearest", k_devt_nearest, (unsigned)gq, DEV_T, 0, h->sorted4.p, pos0, pos1, T, contact_index(ref), ref->hmeta.n_sorted,
               rb0, rb1, P.max_dist * P.max_dist, D.dev.p, D.fix.p, D.d2.p, D.ref_index.p, D.status.p, D.owned.p);
        if (smooth)
            LAUNCH(h, "k_devt_smooth", k_devt_smooth, (unsigned)gq, DEV_T, 0, contact_index(h), pos0, pos1, T, hb0, hb1,
                   P.smooth_radius * P.smooth_radius, D.status.p, D.fix.p, D.smoothed.p);
        LAUNCH(h, "k_devt_target", k_devt_target, (unsigned)std::min(gq, cap_grid), DEV_T, 0, h->sorted4.p, pos0, pos1, T, D.status.p, D.dev.p, v,
               D.d2.p, D.ref_index.p, P.allowance, P.gain, D.target.p, D.acc.p);
    }
    unsigned long long acc[DEVT_ACC_WORDS];
    HIPCHK(h, copy_sync(h, acc, D.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
    const unsigned long long own = acc[0] + acc[1] + acc[2];
    if (own + acc[DEVT_ACC_HALO] > (unsigned long long)(pos1 - pos0) || acc[DEV_ACC_PROUD] > acc[0] || acc[DEV_ACC_BELOW] > acc[0])
        return fail(h, PPP_ERR_HIP, "deviation tile: statistics corrupt");
    if (part) {
        ppp_deviation_tile_stats st = {};
        dev_stats_words(st, N, acc);
        st.owned = (size_t)own; st.evaluated = (size_t)(own + acc[DEVT_ACC_HALO]);
        if (st.matched) st.fix_sum = (long long)acc[DEV_ACC_FIXSUM];
        st.own_lo = T.own_lo; st.own_hi = T.own_hi;
        st.sum_parts = MapParts(h, N).grid;
        *part = st;
    }
    return deviation_copy_out(h, std::min(cap, N), v, deviation, smoothed, ref_index, status, target, owned);
}

/* The merge of ppp_get_deviation_tile's parts (host only).  The integer fields add and fold; hist needs the global span, and
   rms_dev / target_sum are ppp_get_deviation's fixed-order sums (B.46: k_dev_stats's partition into sum_parts contiguous parts
   of the map, inside a part every one of PCON_T threads its strided share in index order, block_tree_sum's tree over the
   threads, the parts in order), which no per-tile number can give: they are computed here from the union of the owned entries. */
int ppp_merge_deviation_tiles(size_t tiles, const ppp_deviation_tile_stats *parts, const double *const *v, const unsigned char *const *status,
                              const double *const *target, const unsigned char *const *owned, ppp_deviation_stats *stats)
{
    if (!tiles || !parts || !v || !status || !target || !owned || !stats) return PPP_ERR_ARG;
    const size_t N = parts[0].n;
    const int grid = parts[0].sum_parts;
    if (N > 0x7fffffffu || grid < 1 || (size_t)grid > std::max<size_t>(1, (N + PCON_T - 1) / PCON_T)) return PPP_ERR_ARG;
    ppp_deviation_stats st = {};
    unsigned long long knmin = 0, kmax = 0, fsum = 0;
    unsigned kd2 = 0;
    std::vector<int> owner(N, -1); /* who owns a point: the one tile whose owned map marks it */
    size_t all_owned = 0;
    for (size_t t = 0; t < tiles; ++t) {
        const ppp_deviation_tile_stats &p = parts[t];
        if (p.n != N || p.sum_parts != grid || (N && (!v[t] || !status[t] || !target[t] || !owned[t]))) return PPP_ERR_ARG;
        if (p.matched + p.too_far + p.no_normal != p.owned || p.proud > p.matched || p.below > p.matched) return PPP_ERR_ARG;
        size_t mine = 0, matched = 0;
        for (size_t i = 0; i < N; ++i) {
            if (!owned[t][i]) continue;
            if (owner[i] >= 0) return PPP_ERR_ARG; /* owned twice */
            owner[i] = (int)t;
            ++mine; matched += status[t][i] == PPP_DEV_MATCHED;
        }
        if (mine != p.owned || matched != p.matched) return PPP_ERR_ARG; /* the part is not the maps' */
        all_owned += mine;
        st.matched += p.matched; st.too_far += p.too_far; st.no_normal += p.no_normal; st.proud += p.proud; st.below += p.below;
        if (p.matched) {
            knmin = std::max(knmin, ordered_key64(-p.min_dev)); kmax = std::max(kmax, ordered_key64(p.max_dev));
            fsum += (unsigned long long)p.fix_sum;
            kd2 = std::max(kd2, ordered_key(p.max_dist2));
        }
    }
    st.n = N; st.dropped = N - all_owned; /* nobody's points: the non-finite ones */
    st.min_dev = st.max_dev = st.mean_dev = st.rms_dev = (double)NAN; st.max_dist2 = NAN;
    double span = 0.0;
    if (st.matched) {
        st.min_dev = -ordered_unkey64(knmin); st.max_dev = ordered_unkey64(kmax);
        st.mean_dev = (double)(long long)fsum / (double)st.matched * (1.0 / DEV_FIXED);
        st.max_dist2 = ordered_unkey(kd2);
        span = fmax(fabs(st.min_dev), fabs(st.max_dev));
    }
    const size_t per = (N + (size_t)grid - 1) / (size_t)grid;
    std::vector<double> s_sq(PCON_T), s_tg(PCON_T);
    double sq_all = 0.0;
    for (size_t g = 0; g < (size_t)grid; ++g) {
        const size_t i0 = g * per, i1 = std::min(N, i0 + per);
        for (size_t t = 0; t < PCON_T; ++t) {
            double sq = 0.0, tg = 0.0;
            for (size_t i = i0 + t; i < i1; i += PCON_T) {
                if (owner[i] < 0 || status[(size_t)owner[i]][i] != PPP_DEV_MATCHED) continue;
                const double x = v[(size_t)owner[i]][i];
                sq += x * x; tg += target[(size_t)owner[i]][i];
                ++st.hist[dev_bin(x, span)];
            }
            s_sq[t] = sq; s_tg[t] = tg;
        }
        for (size_t o = PCON_T / 2; o > 0; o >>= 1)
            for (size_t t = 0; t < o; ++t) { s_sq[t] += s_sq[t + o]; s_tg[t] += s_tg[t + o]; }
        sq_all += s_sq[0]; st.target_sum += s_tg[0];
    }
    if (st.matched) st.rms_dev = std::sqrt(sq_all / (double)st.matched);
    *stats = st;
    return PPP_OK;
}

/* ---- registration of a scan held as slice-range tiles ---- */

/* one tile of a call: the scan's handle, its reference, and what k_regt_terms is launched with */
struct RegtTile {
    ppp_handle h = nullptr, ref = nullptr;
    TileRange own;
    RegtNeed need;
    int pos0 = 0, pos1 = 0, rb0 = 0, rb1 = 0, nref = 0;
    unsigned grid = 1;
    ppp_registration_part part;
    ppp_trimesh mesh = nullptr; /* ppp_register_mesh_tiles: the mesh in the reference's place (ref stays NULL), k_mesht_reg_search's grid */
    unsigned gsearch = 1;
};

/* the tile's pinned memory: REGT_WORDS words coming back, then the 12 doubles of T going out */
static double *regt_pinned_T(const RegtTile &t) { return reinterpret_cast<double *>(t.h->registration.tpin.p + REGT_WORDS); }

/* What a tile needs before its first evaluation: the checks (B.72's, a part handle), both plans, both indices -- the
   reference's index and normal field only where build_ref says so: a handle that stands in several slots is built once --, the
   frame and the shift of the WHOLE clouds (B.90), the positions, the reference's sorted slabs and indexed interval, the
   buffers, and the frame on the device. */
static int regt_prepare(RegtTile &t, const ppp_registration_params &P, IcpFrame F, bool build_ref)
{
    ppp_handle h = t.h, ref = t.ref;
    HIPCHK(h, hipSetDevice(h->device));
    if (ref->device != h->device) return fail(h, PPP_ERR_ARG, "registration tile: the tile and its reference are on different devices");
    int rc = deviation_side_cloud(h, ref, "registration tile: the reference", true);
    if (rc) return rc;
    if (ref != h) { rc = deviation_side_cloud(h, h, "registration tile: the scan", true); if (rc) return rc; }
    int shift = icp_shift(h->n, F.md2);
    if (shift < 16) return fail(h, PPP_ERR_ARG, "registration tile: fewer than 16 fractional bits are left (n max_dist^2 too large): the integer sums could overflow");
    rc = tile_range(h, 0.f, t.own);
    if (rc) return rc;
    if (build_ref) { rc = deviation_side_index(h, ref, "registration tile: the reference", false); if (rc) return rc; }
    if (ref != h) { rc = deviation_side_index(h, h, "registration tile: the scan", false); if (rc) return rc; }
    /* B.90: the whole reference's bounds.  A whole-cloud handle answers ppp_minmax with them (registration_setup reads the same
       block); a range handle's launches see its part only and are handed the whole cloud's bounds cached with its plan: those */
    if (!ref->ranged) {
        rc = fetch_meta(ref);
        if (rc) return ref == h ? rc : fail(h, rc, std::string("registration tile: the reference: ") + ref->err);
    }
    frame_from_bounds(ref->ranged ? ref->h_mn : ref->hmeta.mn, ref->ranged ? ref->h_mx : ref->hmeta.mx, (double)P.max_dist, shift, F.c, &F.Ln, &F.scale);
    if (build_ref) { rc = reference_normals(h, ref, "registration tile"); if (rc) return rc; }
    rc = tile_positions(h, t.own, t.pos0, t.pos1);
    if (rc) return rc;
    sorted_slabs(ref, t.rb0, t.rb1);
    t.nref = ref->hmeta.n_sorted;
    t.need = RegtNeed{ref->incl_lo, ref->incl_hi, 1.0001f * (P.max_dist + ref->P.normal_radius), ref->ranged && ref->incl_lo > ref->h_mn[0],
                      ref->ranged && ref->incl_hi < ref->h_mx[0]};
    t.grid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)(t.pos1 - t.pos0) + ICP_T - 1) / ICP_T, 2 * (size_t)h->num_cus));
    ppp_registration_part &p = t.part;
    p = ppp_registration_part{};
    p.evaluated = (size_t)(t.pos1 - t.pos0);
    p.own_lo = t.own.own_lo; p.own_hi = t.own.own_hi;
    p.n = h->n; p.shift = shift;
    for (int d = 0; d < 3; ++d) p.centre[d] = F.c[d];
    p.length = F.Ln;
    auto &G = h->registration;
    HIPCHK(h, G.T.ensure(12)); HIPCHK(h, G.acc.ensure(REGT_WORDS)); HIPCHK(h, G.tframe.ensure(1)); HIPCHK(h, G.tpin.ensure(REGT_WORDS + 12));
    HIPCHK(h, copy_sync(h, G.tframe.p, &F, sizeof(F), hipMemcpyHostToDevice));
    return PPP_OK;
}

/* one evaluation of a tile at T, enqueued on its handle's stream: T to the device, the words cleared, k_regt_terms, the words
   back to pinned memory.  Nobody waits here. */
static int regt_enqueue(RegtTile &t, const double *T)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    memcpy(regt_pinned_T(t), T, 12 * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(G.T.p, regt_pinned_T(t), 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, REGT_WORDS * sizeof(unsigned long long), h->stream));
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_regt_terms", k_regt_terms, t.grid, ICP_T, 0, h->sorted4.p, t.pos0, t.pos1, t.own, contact_index(t.ref), t.nref, t.rb0, t.rb1, t.need,
               G.tframe.p, G.T.p, G.acc.p);
    HIPCHK(h, hipMemcpyAsync(G.tpin.p, G.acc.p, REGT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* the wait for what a tile's stream holds */
static int regt_wait(RegtTile &t)
{
    HIPCHK(t.h, hipSetDevice(t.h->device));
    HIPCHK(t.h, hipStreamSynchronize(t.h->stream));
    return PPP_OK;
}

/* the refusal of an evaluation whose moved queries left what the reference indexes (B.89); w: the call's name */
static std::string regt_refusal(const char *w, unsigned long long queries)
{
    return std::string(w) + ": " + std::to_string(queries) + " moved queries reach beyond the reference's indexed slice range "
           "(max_dist + normal_radius around the moved point): raise range_margin of the reference's handle";
}

/* the wait for a tile's evaluation, and its row: the refusal (B.89), the words' sanity, the terms */
static int regt_collect(RegtTile &t, const double *T, ppp_registration_row *row)
{
    ppp_handle h = t.h;
    int rc = regt_wait(t);
    if (rc) return rc;
    const unsigned long long *w = h->registration.tpin.p;
    if (w[REGT_REFUSED]) return fail(h, PPP_ERR_CAPACITY, regt_refusal("registration tile", w[REGT_REFUSED]));
    if (w[REGT_OWNED] > (unsigned long long)(t.pos1 - t.pos0) || w[ICP_PAIRS] > w[REGT_OWNED]) return fail(h, PPP_ERR_HIP, "registration tile: sums corrupt");
    t.part.owned = (size_t)w[REGT_OWNED];
    *row = ppp_registration_row{};
    icp_row_terms(row, T, w);
    return PPP_OK;
}

/* the checks every tiled call makes before it looks at a handle: the parameters and the transform (errors on h) */
static int regt_call_ok(ppp_handle h, const ppp_registration_params *rp, const double *T0, IcpFrame &F, double *T)
{
    if (!h) return PPP_ERR_ARG;
    if (!rp) return fail(h, PPP_ERR_ARG, "registration tile: no parameters");
    const int rc = registration_params_ok(h, *rp, F);
    return rc ? rc : opening_transform(h, "registration tile", T0, T);
}

int ppp_get_registration_terms_tile(ppp_handle h, ppp_handle ref, const ppp_registration_params *rp, const double *T12, ppp_registration_row *row,
                                    ppp_registration_part *part)
{
    IcpFrame F = {};
    double T[12];
    int rc = regt_call_ok(h, rp, T12, F, T);
    if (rc) return rc;
    if (!ref) return fail(h, PPP_ERR_ARG, "registration tile: no reference handle");
    RegtTile t;
    t.h = h; t.ref = ref;
    rc = regt_prepare(t, *rp, F, true);
    if (rc) return rc;
    rc = regt_enqueue(t, T);
    if (rc) return rc;
    ppp_registration_row r;
    rc = regt_collect(t, T, &r);
    if (rc) return rc;
    if (row) *row = r;
    if (part) *part = t.part;
    return PPP_OK;
}

int ppp_merge_registration_terms(const ppp_registration_row *rows, const ppp_registration_part *parts, size_t count, const double *T12,
                                 ppp_registration_row *out_row, ppp_registration_part *out_part)
{
    if (!rows || !parts || !count || !out_row) return PPP_ERR_ARG;
    std::vector<size_t> by_lo;
    for (size_t i = 0; i < count; ++i) {
        if (!regt_same_frame(parts[i], parts[0])) return PPP_ERR_ARG;
        if (parts[i].own_lo < parts[i].own_hi) by_lo.push_back(i); /* (an empty interval, or one with a NaN, overlaps nothing) */
    }
    std::sort(by_lo.begin(), by_lo.end(), [&](size_t a, size_t b) { return parts[a].own_lo < parts[b].own_lo; });
    for (size_t k = 1; k < by_lo.size(); ++k)
        if (parts[by_lo[k]].own_lo < parts[by_lo[k - 1]].own_hi) return PPP_ERR_ARG; /* half-open: equal ends meet */
    unsigned long long acc[ICP_WORDS] = {};
    ppp_registration_part m = parts[0];
    m.owned = m.evaluated = 0; m.own_lo = INFINITY; m.own_hi = -INFINITY;
    for (size_t i = 0; i < count; ++i) {
        const ppp_registration_row &r = rows[i];
        acc[ICP_PAIRS] += (unsigned long long)r.pairs;
        for (int w = 0; w < 21; ++w) acc[ICP_A + w] += (unsigned long long)r.A[w];
        for (int w = 0; w < 6; ++w) acc[ICP_B + w] += (unsigned long long)r.b[w];
        acc[ICP_E] += (unsigned long long)r.E;
        m.owned += parts[i].owned; m.evaluated += parts[i].evaluated;
        if (parts[i].own_lo < parts[i].own_hi) { m.own_lo = std::min(m.own_lo, parts[i].own_lo); m.own_hi = std::max(m.own_hi, parts[i].own_hi); }
    }
    *out_row = ppp_registration_row{};
    icp_row_terms(out_row, T12 ? T12 : ICP_IDENTITY, acc);
    if (out_part) *out_part = m;
    return PPP_OK;
}

int ppp_registration_step(const ppp_registration_row *row, const ppp_registration_part *part, double lock_eps, const double *T12, double *T12_out,
                          int *locked, double *step2)
{
    if (!row || !part || !T12_out || !(lock_eps > 0.0 && lock_eps < 1.0) || !(part->length > 0.0 && part->length < INFINITY)) return PPP_ERR_ARG;
    double T[12], Tn[12];
    memcpy(T, T12 ? T12 : row->T, sizeof(T));
    memcpy(Tn, T, sizeof(Tn));
    int mask;
    double s2;
    const int rc = regt_step(*row, part->centre, part->length, lock_eps, T, Tn, &mask, &s2);
    memcpy(T12_out, Tn, sizeof(Tn));
    if (locked) *locked = mask;
    if (step2) *step2 = s2;
    return rc;
}

/* a tiled loop's call: its name in the messages, where a failing tile's slot goes, the tiles, their rows and parts of the evaluation at hand and the whole they merge to */
struct RegtCall {
    const char *what;
    ppp_register_tiles_stats *stats;
    std::vector<RegtTile> tiles;
    std::vector<ppp_registration_row> part_rows;
    std::vector<ppp_registration_part> parts;
    ppp_registration_part whole;
    int failed(size_t i, int code) const { if (stats) stats->failed_tile = (int)i; return code; }
};

/* The opening of a tiled loop behind its parameters' checks (errors on the first handle): rows that are missing, the handles,
   and every tile prepared, with `also`, the call's own step per tile, behind regt_prepare */
static int regt_open(RegtCall &call, const ppp_handle *hs, const ppp_handle *refs, size_t count, const ppp_registration_params &P, const IcpFrame &F,
                     bool rows_missing, const std::function<int(RegtTile &, size_t)> &also = nullptr)
{
    ppp_handle h0 = hs[0];
    const std::string w(call.what);
    if (rows_missing) return fail(h0, PPP_ERR_ARG, w + ": rows is NULL with row_cap > 0");
    for (size_t i = 0; i < count; ++i) {
        if (!hs[i] || !refs[i]) return fail(h0, PPP_ERR_ARG, w + ": a NULL handle");
        for (size_t k = 0; k < i; ++k) if (hs[k] == hs[i]) return fail(h0, PPP_ERR_ARG, w + ": a scan handle stands in two slots");
    }
    call.tiles.assign(count, RegtTile()); call.part_rows.resize(count); call.parts.resize(count);
    for (size_t i = 0; i < count; ++i) {
        RegtTile &t = call.tiles[i];
        t.h = hs[i]; t.ref = refs[i];
        bool first = true; /* the reference's index and normal field: once per reference handle */
        for (size_t k = 0; k < i; ++k) first = first && refs[k] != refs[i];
        int rc = regt_prepare(t, P, F, first);
        if (!rc && also) rc = also(t, i);
        if (rc) return call.failed(i, rc);
    }
    return PPP_OK;
}

/* One pass over the tiles: `enqueue` on every tile's stream, then every tile waited for (`wait`, the tile and its slot, where
   the wait does more than regt_wait), whatever an earlier one answered; the first error is the call's */
static int regt_pass(RegtCall &call, const std::function<int(RegtTile &)> &enqueue, const std::function<int(RegtTile &, size_t)> &wait = nullptr)
{
    for (size_t i = 0; i < call.tiles.size(); ++i) { const int e = enqueue(call.tiles[i]); if (e) return call.failed(i, e); }
    int first_rc = PPP_OK;
    for (size_t i = 0; i < call.tiles.size(); ++i) {
        const int e = wait ? wait(call.tiles[i], i) : regt_wait(call.tiles[i]);
        if (e && !first_rc) first_rc = call.failed(i, e);
    }
    return first_rc;
}

/* the tiles' rows of one evaluation at T as the whole cloud's (B.91), with the checks the loops make of it */
static int regt_merged(ppp_handle h0, RegtCall &call, const double *T, ppp_registration_row &rw)
{
    const int rc = ppp_merge_registration_terms(call.part_rows.data(), call.parts.data(), call.parts.size(), T, &rw, &call.whole);
    if (rc) return fail(h0, rc, "registration tiles: the tiles' ranges overlap, or the tiles do not hold one scan against one reference");
    if (rw.pairs > call.whole.owned) return fail(h0, PPP_ERR_HIP, "registration tiles: sums corrupt");
    return PPP_OK;
}

/* The tiled loop (B.93): ppp_register's chain with the host in the place of k_reg_step (regt_loop); an evaluation is one
   k_regt_terms per tile and one wait per tile. */
int ppp_register_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count, const ppp_registration_params *rp, const double *T0_12,
                       ppp_registration_row *rows, size_t row_cap, ppp_register_tiles_stats *stats)
{
    if (stats) { *stats = ppp_register_tiles_stats{}; stats->failed_tile = -1; }
    if (!hs || !refs || !count || !hs[0]) return PPP_ERR_ARG;
    ppp_handle h0 = hs[0];
    IcpFrame F = {};
    double T[12];
    int rc = regt_call_ok(h0, rp, T0_12, F, T);
    if (rc) return rc;
    const ppp_registration_params P = *rp;
    RegtCall call = {"registration tiles", stats};
    rc = regt_open(call, hs, refs, count, P, F, !rows && row_cap);
    if (rc) return rc;
    std::vector<ppp_registration_row> R;
    IcpCtl C = {};
    rc = regt_loop(P, F, T, R, C, call.whole, [&](int, ppp_registration_row &rw) {
        const int e = regt_pass(call, [&](RegtTile &t) { return regt_enqueue(t, T); }, [&](RegtTile &t, size_t i) {
            const int ec = regt_collect(t, T, &call.part_rows[i]);
            call.parts[i] = t.part;
            return ec;
        });
        return e ? e : regt_merged(h0, call, T, rw);
    });
    if (rc) return rc;
    if (stats) stats->reg = registration_stats(R, C, call.whole.n, call.whole.owned, call.whole.shift, call.whole.centre, call.whole.length);
    const size_t k = std::min(row_cap, (size_t)C.steps + 1);
    if (rows && k) memcpy(rows, R.data(), k * sizeof(ppp_registration_row));
    return PPP_OK;
}

/* ---- trimmed registration of a scan held as slice-range tiles ---- */

int ppp_trim_select(const unsigned int *hist, size_t bins, size_t rank, unsigned int *bin, size_t *rank_in_bin)
{
    if (!hist || !bin || !rank_in_bin) return PPP_ERR_ARG;
    *bin = 0; *rank_in_bin = 0;
    size_t below = 0;
    for (size_t b = 0; rank && b < bins; ++b) {
        if (rank <= below + hist[b]) { *bin = (unsigned)b; *rank_in_bin = rank - below; break; } /* (rank > below: no earlier bin reached it) */
        below += hist[b];
    }
    return PPP_OK;
}

size_t ppp_trim_rank(double keep, size_t paired) { return trim_rank(keep, paired); }

/* a tile's pinned memory behind ppp_register_tiles' (the words back, T out): one word going out -- the merged prefix, then tau --
   and the block coming back: the two words and a histogram of at most TRIM_B0 bins */
static unsigned *trimt_pinned_word(const RegtTile &t) { return reinterpret_cast<unsigned *>(t.h->registration.tpin.p + REGT_WORDS + 12); }
static unsigned *trimt_pinned_hist(const RegtTile &t) { return reinterpret_cast<unsigned *>(t.h->registration.tpin.p + REGT_WORDS + 13); }
static const size_t TRIMT_PIN_WORDS = REGT_WORDS + 13 + (TRIMT_HEAD + TRIM_B0) / 2;
static int trimt_positions(const RegtTile &t) { return t.pos1 - t.pos0; }

/* the buffers of a tile behind regt_prepare: partner and key per position, the two words and the three histograms, the word
   the host writes, and where the caller wants a map of this tile, status | owned and d2 by cloud index */
static int trimt_prepare(RegtTile &t, bool maps)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    const size_t np = std::max<size_t>((size_t)trimt_positions(t), 1), N1 = std::max<size_t>(h->n, 1);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, G.partner.ensure(np)); HIPCHK(h, G.key.ensure(np)); HIPCHK(h, G.hist.ensure(TRIMT_HEAD + TRIM_WORDS)); HIPCHK(h, G.cuts.ensure(2));
    HIPCHK(h, G.tpin.ensure(TRIMT_PIN_WORDS));
    if (maps) { HIPCHK(h, G.tstatus.ensure(2 * N1)); HIPCHK(h, G.td2.ensure(N1)); }
    return PPP_OK;
}

/* the first pass of an evaluation at T, enqueued on the tile's stream: T to the device, the histograms and the words cleared,
   k_trimt_pair, the two words and the top digits' histogram back to pinned memory.  Nobody waits here. */
static int trimt_enqueue_pair(RegtTile &t, const double *T)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    memcpy(regt_pinned_T(t), T, 12 * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(G.T.p, regt_pinned_T(t), 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(G.hist.p, 0, (TRIMT_HEAD + TRIM_WORDS) * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, ICP_WORDS * sizeof(unsigned long long), h->stream));
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_trimt_pair", k_trimt_pair, t.grid, TRIM_T, 0, h->sorted4.p, t.pos0, t.pos1, t.own, contact_index(t.ref), t.nref, t.rb0, t.rb1, t.need,
               G.tframe.p, G.T.p, G.partner.p, G.key.p, G.hist.p);
    HIPCHK(h, hipMemcpyAsync(trimt_pinned_hist(t), G.hist.p, (TRIMT_HEAD + TRIM_B0) * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* pass 1 or 2: the merged prefix to the device, k_trimt_narrow over the stored keys, that digit's histogram back */
static int trimt_enqueue_narrow(RegtTile &t, int pass, unsigned prefix)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    unsigned *next = G.hist.p + TRIMT_HEAD + (pass == 1 ? TRIM_B0 : TRIM_B0 + TRIM_B1);
    *trimt_pinned_word(t) = prefix;
    HIPCHK(h, hipMemcpyAsync(G.cuts.p, trimt_pinned_word(t), sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    if (t.pos1 > t.pos0) {
        if (pass == 1) LAUNCH(h, "k_trimt_narrow<1>", k_trimt_narrow<1>, t.grid, TRIM_T, 0, G.key.p, trimt_positions(t), G.cuts.p, next);
        else LAUNCH(h, "k_trimt_narrow<2>", k_trimt_narrow<2>, t.grid, TRIM_T, 0, G.key.p, trimt_positions(t), G.cuts.p, next);
    }
    HIPCHK(h, hipMemcpyAsync(trimt_pinned_hist(t), next, (pass == 1 ? TRIM_B1 : TRIM_B2) * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* the sums: tau to the device, k_trimt_terms, the 29 words back */
static int trimt_enqueue_terms(RegtTile &t, unsigned tau)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    *trimt_pinned_word(t) = tau;
    HIPCHK(h, hipMemcpyAsync(G.cuts.p, trimt_pinned_word(t), sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_trimt_terms", k_trimt_terms, t.grid, TRIM_T, 0, h->sorted4.p, t.pos0, t.pos1, contact_index(t.ref), G.tframe.p, G.T.p, G.partner.p,
               G.key.p, G.cuts.p, G.acc.p);
    HIPCHK(h, hipMemcpyAsync(G.tpin.p, G.acc.p, ICP_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* behind the loop: the tile's maps filled with DROPPED / NaN / 0, then k_trimt_scatter over the keys the last evaluation left */
static int trimt_enqueue_scatter(RegtTile &t, unsigned tau, bool none)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    const size_t N1 = std::max<size_t>(h->n, 1);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(G.tstatus.p, PPP_TRIM_DROPPED, N1, h->stream));
    HIPCHK(h, hipMemsetAsync(G.tstatus.p + N1, 0, N1, h->stream));
    HIPCHK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(G.td2.p), (int)TRIM_NAN, N1, h->stream));
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_trimt_scatter", k_trimt_scatter, t.grid, TRIM_T, 0, h->sorted4.p, t.pos0, t.pos1, G.key.p, tau, none ? 1 : 0, (int)N1, G.tstatus.p,
               G.td2.p, G.tstatus.p + N1);
    return PPP_OK;
}

/* the first min(cap, n) entries of the maps the caller gave for this tile (each copy waits for the tile's stream) */
static int trimt_copy_maps(RegtTile &t, unsigned char *status, float *d2, unsigned char *owned, size_t cap)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    const size_t N1 = std::max<size_t>(h->n, 1), m = std::min(cap, h->n);
    if (!m || !(status || d2 || owned)) return PPP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (status) HIPCHK(h, copy_sync(h, status, G.tstatus.p, m, hipMemcpyDeviceToHost));
    if (d2) HIPCHK(h, copy_sync(h, d2, G.td2.p, m * sizeof(float), hipMemcpyDeviceToHost));
    if (owned) HIPCHK(h, copy_sync(h, owned, G.tstatus.p + N1, m, hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* The tiled trimmed loop (B.97-B.99): regt_loop, an evaluation being four passes over the tiles -- k_trimt_pair,
   k_trimt_narrow<1>, k_trimt_narrow<2>, k_trimt_terms --, each enqueued on every tile's stream and waited for tile by tile; between
   them the host adds the tiles' histograms, selects the digit on the sum (ppp_trim_select) and sends the next pass the merged
   prefix, or tau.  An evaluation that finds no pair in any tile ends behind its first pass. */
int ppp_register_trimmed_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count, const ppp_trimmed_registration_params *tp, const double *T0_12,
                               ppp_trimmed_registration_row *rows, size_t row_cap, unsigned char *const *status, float *const *d2,
                               unsigned char *const *owned, size_t cap, ppp_register_tiles_stats *stats)
{
    if (stats) { *stats = ppp_register_tiles_stats{}; stats->failed_tile = -1; }
    if (!hs || !refs || !count || !hs[0]) return PPP_ERR_ARG;
    ppp_handle h0 = hs[0];
    if (!tp) return fail(h0, PPP_ERR_ARG, "trimmed registration tiles: no parameters");
    IcpFrame F = {};
    double T[12];
    int rc = regt_call_ok(h0, &tp->icp, T0_12, F, T);
    if (rc) return rc;
    const double keep = tp->keep;
    if (!(keep > 0.0 && keep <= 1.0)) return fail(h0, PPP_ERR_ARG, "trimmed registration tiles: keep must be in (0, 1]");
    const ppp_registration_params P = tp->icp;
    auto map_of = [&](auto *const *maps, size_t i) { return maps ? maps[i] : nullptr; };
    auto wants_maps = [&](size_t i) { return map_of(status, i) || map_of(d2, i) || map_of(owned, i); };
    RegtCall call = {"trimmed registration tiles", stats};
    rc = regt_open(call, hs, refs, count, P, F, !rows && row_cap, [&](RegtTile &t, size_t i) { return trimt_prepare(t, wants_maps(i)); });
    if (rc) return rc;
    std::vector<RegtTile> &tiles = call.tiles;
    /* the tiles' histograms of `bins` bins, behind the wait, added bin by bin: a bin's sum is at most the scan's points */
    std::vector<unsigned> H(TRIM_B0);
    auto merge_hist = [&](size_t skip, size_t bins) {
        std::fill(H.begin(), H.end(), 0u);
        for (size_t i = 0; i < count; ++i) {
            const unsigned *w = trimt_pinned_hist(tiles[i]) + skip;
            for (size_t b = 0; b < bins; ++b) H[b] += w[b];
        }
    };
    struct Cut { size_t paired; unsigned tau; };
    std::vector<Cut> cuts;
    std::vector<ppp_registration_row> R;
    IcpCtl C = {};
    rc = regt_loop(P, F, T, R, C, call.whole, [&](int, ppp_registration_row &rw) {
        int e = regt_pass(call, [&](RegtTile &t) { return trimt_enqueue_pair(t, T); });
        if (e) return e;
        size_t paired = 0;
        for (size_t i = 0; i < count; ++i) {
            RegtTile &t = tiles[i];
            const unsigned *w = trimt_pinned_hist(t);
            if (w[TRIMT_REFUSED]) return call.failed(i, fail(t.h, PPP_ERR_CAPACITY, regt_refusal(call.what, w[TRIMT_REFUSED])));
            size_t mine = 0;
            for (size_t b = 0; b < TRIM_B0; ++b) mine += w[TRIMT_HEAD + b];
            if (w[TRIMT_OWNED] > (unsigned)trimt_positions(t) || mine > w[TRIMT_OWNED]) return call.failed(i, fail(t.h, PPP_ERR_HIP, "trimmed registration tiles: histogram corrupt"));
            t.part.owned = w[TRIMT_OWNED];
            call.parts[i] = t.part;
            call.part_rows[i] = ppp_registration_row{};
            paired += mine;
        }
        Cut cut = {paired, TRIM_NAN};
        if (paired) { /* B.78 on the merged histograms; without a pair the evaluation ends here: kept 0, no sums */
            merge_hist(TRIMT_HEAD, TRIM_B0);
            unsigned bin, prefix;
            size_t rank;
            ppp_trim_select(H.data(), TRIM_B0, trim_rank(keep, paired), &bin, &rank);
            if (!rank) return fail(h0, PPP_ERR_HIP, "trimmed registration tiles: cut corrupt");
            prefix = bin << 21;
            for (int pass = 1; pass <= 2; ++pass) {
                const size_t bins = pass == 1 ? TRIM_B1 : TRIM_B2;
                e = regt_pass(call, [&](RegtTile &t) { return trimt_enqueue_narrow(t, pass, prefix); });
                if (e) return e;
                merge_hist(0, bins);
                ppp_trim_select(H.data(), bins, rank, &bin, &rank);
                if (!rank) return fail(h0, PPP_ERR_HIP, "trimmed registration tiles: cut corrupt");
                prefix |= pass == 1 ? bin << 10 : bin;
            }
            cut.tau = prefix;
            e = regt_pass(call, [&](RegtTile &t) { return trimt_enqueue_terms(t, cut.tau); });
            if (e) return e;
            for (size_t i = 0; i < count; ++i) {
                const unsigned long long *w = tiles[i].h->registration.tpin.p;
                if (w[ICP_PAIRS] > call.parts[i].owned) return call.failed(i, fail(tiles[i].h, PPP_ERR_HIP, "trimmed registration tiles: sums corrupt"));
                icp_row_terms(&call.part_rows[i], T, w);
            }
        }
        e = regt_merged(h0, call, T, rw);
        if (e) return e;
        if (rw.pairs > paired || (paired && rw.pairs < trim_rank(keep, paired))) return fail(h0, PPP_ERR_HIP, "trimmed registration tiles: cut corrupt");
        cuts.push_back(cut);
        return (int)PPP_OK;
    });
    if (rc) return rc;
    const size_t last = (size_t)C.steps;
    /* B.99: the maps of the last evaluation -- its keys are the ones the tiles hold --, every tile's launch before any copy */
    for (size_t i = 0; i < count; ++i)
        if (wants_maps(i)) {
            rc = trimt_enqueue_scatter(tiles[i], cuts[last].tau, cuts[last].paired == 0);
            if (rc) return call.failed(i, rc);
        }
    for (size_t i = 0; i < count; ++i) {
        rc = trimt_copy_maps(tiles[i], map_of(status, i), map_of(d2, i), map_of(owned, i), cap);
        if (rc) return call.failed(i, rc);
    }
    if (stats) stats->reg = registration_stats(R, C, call.whole.n, call.whole.owned, call.whole.shift, call.whole.centre, call.whole.length);
    const size_t k = std::min(row_cap, last + 1);
    for (size_t i = 0; rows && i < k; ++i) trimmed_row(rows[i], R[i], cuts[i].paired, cuts[i].tau);
    return PPP_OK;
}

/* ---- robust registration of a scan held as slice-range tiles ---- */

double ppp_robust_sigma(unsigned int median_bits, int none, double sigma_min) { return rob_sigma(median_bits, none != 0, sigma_min); }

double ppp_robust_weight(double r, double cs, double tune) { return rob_weight(r, cs, tune); }

/* the buffers of a tile behind regt_prepare: trimt_prepare's, the residual per position, and where the caller wants a map of this
   tile the residual map by cloud index beside status | owned and the weight */
static int robt_prepare(RegtTile &t, bool maps)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    const int rc = trimt_prepare(t, maps);
    if (rc) return rc;
    HIPCHK(h, G.rres.ensure(std::max<size_t>((size_t)trimt_positions(t), 1)));
    if (maps) HIPCHK(h, G.rresid.ensure(std::max<size_t>(h->n, 1)));
    return PPP_OK;
}

/* the first pass of an evaluation at T, enqueued on the tile's stream: T to the device, the histograms and the words cleared,
   k_robt_pair, the two words and the top digits' histogram back to pinned memory.  Nobody waits here. */
static int robt_enqueue_pair(RegtTile &t, const double *T)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    memcpy(regt_pinned_T(t), T, 12 * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(G.T.p, regt_pinned_T(t), 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(G.hist.p, 0, (TRIMT_HEAD + TRIM_WORDS) * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, ROB_WORDS * sizeof(unsigned long long), h->stream));
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_robt_pair", k_robt_pair, t.grid, TRIM_T, 0, h->sorted4.p, t.pos0, t.pos1, t.own, contact_index(t.ref), t.nref, t.rb0, t.rb1, t.need,
               G.tframe.p, G.T.p, G.partner.p, G.rres.p, G.key.p, G.hist.p);
    HIPCHK(h, hipMemcpyAsync(trimt_pinned_hist(t), G.hist.p, (TRIMT_HEAD + TRIM_B0) * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* the sums: the merged tau to the device, k_robt_terms, the 30 words back */
static int robt_enqueue_terms(RegtTile &t, unsigned tau, const RobScale &S)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    *trimt_pinned_word(t) = tau;
    HIPCHK(h, hipMemcpyAsync(G.cuts.p, trimt_pinned_word(t), sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_robt_terms", k_robt_terms, t.grid, TRIM_T, 0, h->sorted4.p, t.pos0, t.pos1, contact_index(t.ref), G.tframe.p, S, G.T.p, G.partner.p,
               G.rres.p, G.key.p, G.cuts.p, G.acc.p);
    HIPCHK(h, hipMemcpyAsync(G.tpin.p, G.acc.p, ROB_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* behind the loop: the tile's maps filled with DROPPED / NaN / NaN / 0 (k_robt_fill: a double NaN is no memset pattern), then
   k_robt_scatter over the keys and the residuals the last evaluation left */
static int robt_enqueue_scatter(RegtTile &t, double cs, double tune, bool none)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    const size_t N1 = std::max<size_t>(h->n, 1);
    HIPCHK(h, hipSetDevice(h->device));
    LAUNCH(h, "k_robt_fill", k_robt_fill, (unsigned)std::min<size_t>((N1 + TRIM_T - 1) / TRIM_T, 2 * (size_t)h->num_cus), TRIM_T, 0, (int)N1, G.tstatus.p,
           G.td2.p, G.rresid.p, G.tstatus.p + N1);
    if (t.pos1 > t.pos0)
        LAUNCH(h, "k_robt_scatter", k_robt_scatter, t.grid, TRIM_T, 0, h->sorted4.p, t.pos0, t.pos1, G.key.p, G.rres.p, cs, tune, none ? 1 : 0, (int)N1,
               G.tstatus.p, G.td2.p, G.rresid.p, G.tstatus.p + N1);
    return PPP_OK;
}

/* the first min(cap, n) entries of the residual map, where the caller gave one for this tile (the copy waits for the tile's stream) */
static int robt_copy_residual(RegtTile &t, double *residual, size_t cap)
{
    ppp_handle h = t.h;
    const size_t m = std::min(cap, h->n);
    if (!m || !residual) return PPP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, copy_sync(h, residual, h->registration.rresid.p, m * sizeof(double), hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* The tiled robust loop (B.106-B.110): regt_loop, an evaluation being four passes over the tiles -- k_robt_pair,
   k_trimt_narrow<1>, k_trimt_narrow<2>, k_robt_terms --, each enqueued on every tile's stream and waited for tile by tile; between
   them the host adds the tiles' histograms, selects the digit of the median on the sum (ppp_trim_select at rank
   ppp_trim_rank(0.5, paired)) and sends the next pass the merged prefix, or tau.  The row the step reads carries `used` in
   pairs, as word 0 of the whole-cloud chain does; the row that is recorded carries paired.  An evaluation that finds no pair in
   any tile ends behind its first pass. */
int ppp_register_robust_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count, const ppp_robust_registration_params *bp, const double *T0_12,
                              ppp_robust_registration_row *rows, size_t row_cap, unsigned char *const *status, float *const *weight,
                              double *const *residual, unsigned char *const *owned, size_t cap, ppp_register_tiles_stats *stats)
{
    if (stats) { *stats = ppp_register_tiles_stats{}; stats->failed_tile = -1; }
    if (!hs || !refs || !count || !hs[0]) return PPP_ERR_ARG;
    ppp_handle h0 = hs[0];
    if (!bp) return fail(h0, PPP_ERR_ARG, "robust registration tiles: no parameters");
    IcpFrame F = {};
    double T[12];
    int rc = regt_call_ok(h0, &bp->icp, T0_12, F, T);
    if (rc) return rc;
    if (!(bp->tune > 0.0)) return fail(h0, PPP_ERR_ARG, "robust registration tiles: tune must be > 0 (+INFINITY: every weight is 1)");
    if (!(bp->sigma_min >= 0.0 && std::isfinite(bp->sigma_min))) return fail(h0, PPP_ERR_ARG, "robust registration tiles: sigma_min must be finite and >= 0");
    const ppp_registration_params P = bp->icp;
    const RobScale S = {bp->tune, bp->sigma_min};
    auto map_of = [&](auto *const *maps, size_t i) { return maps ? maps[i] : nullptr; };
    auto wants_maps = [&](size_t i) { return map_of(status, i) || map_of(weight, i) || map_of(residual, i) || map_of(owned, i); };
    RegtCall call = {"robust registration tiles", stats};
    rc = regt_open(call, hs, refs, count, P, F, !rows && row_cap, [&](RegtTile &t, size_t i) { return robt_prepare(t, wants_maps(i)); });
    if (rc) return rc;
    std::vector<RegtTile> &tiles = call.tiles;
    /* the tiles' histograms of `bins` bins, behind the wait, added bin by bin: a bin's sum is at most the scan's points */
    std::vector<unsigned> H(TRIM_B0);
    auto merge_hist = [&](size_t skip, size_t bins) {
        std::fill(H.begin(), H.end(), 0u);
        for (size_t i = 0; i < count; ++i) {
            const unsigned *w = trimt_pinned_hist(tiles[i]) + skip;
            for (size_t b = 0; b < bins; ++b) H[b] += w[b];
        }
    };
    /* what an evaluation leaves beside its row: B.107's scale and the two words the row does not hold */
    struct Scale { size_t paired, used; unsigned tau; double sigma; long long weight_sum; };
    std::vector<Scale> scales;
    std::vector<ppp_registration_row> R;
    IcpCtl C = {};
    rc = regt_loop(P, F, T, R, C, call.whole, [&](int, ppp_registration_row &rw) {
        int e = regt_pass(call, [&](RegtTile &t) { return robt_enqueue_pair(t, T); });
        if (e) return e;
        size_t paired = 0;
        for (size_t i = 0; i < count; ++i) {
            RegtTile &t = tiles[i];
            const unsigned *w = trimt_pinned_hist(t);
            if (w[TRIMT_REFUSED]) return call.failed(i, fail(t.h, PPP_ERR_CAPACITY, regt_refusal(call.what, w[TRIMT_REFUSED])));
            size_t mine = 0;
            for (size_t b = 0; b < TRIM_B0; ++b) mine += w[TRIMT_HEAD + b];
            if (w[TRIMT_OWNED] > (unsigned)trimt_positions(t) || mine > w[TRIMT_OWNED]) return call.failed(i, fail(t.h, PPP_ERR_HIP, "robust registration tiles: histogram corrupt"));
            t.part.owned = w[TRIMT_OWNED];
            call.parts[i] = t.part;
            call.part_rows[i] = ppp_registration_row{};
            paired += mine;
        }
        Scale sc = {paired, 0, TRIM_NAN, rob_sigma(TRIM_NAN, true, S.sigma_min), 0};
        if (paired) { /* B.102 on the merged histograms; without a pair the evaluation ends here: used 0, no sums */
            merge_hist(TRIMT_HEAD, TRIM_B0);
            unsigned bin, prefix;
            size_t rank;
            ppp_trim_select(H.data(), TRIM_B0, trim_rank(ROB_KEEP, paired), &bin, &rank);
            if (!rank) return fail(h0, PPP_ERR_HIP, "robust registration tiles: median corrupt");
            prefix = bin << 21;
            for (int pass = 1; pass <= 2; ++pass) {
                const size_t bins = pass == 1 ? TRIM_B1 : TRIM_B2;
                e = regt_pass(call, [&](RegtTile &t) { return trimt_enqueue_narrow(t, pass, prefix); });
                if (e) return e;
                merge_hist(0, bins);
                ppp_trim_select(H.data(), bins, rank, &bin, &rank);
                if (!rank) return fail(h0, PPP_ERR_HIP, "robust registration tiles: median corrupt");
                prefix |= pass == 1 ? bin << 10 : bin;
            }
            sc.tau = prefix;
            sc.sigma = rob_sigma(sc.tau, false, S.sigma_min);
            e = regt_pass(call, [&](RegtTile &t) { return robt_enqueue_terms(t, sc.tau, S); });
            if (e) return e;
            unsigned long long wsum = 0; /* B.108: word 29 adds as the 29 in front of it do, two's complement */
            for (size_t i = 0; i < count; ++i) {
                const unsigned long long *w = tiles[i].h->registration.tpin.p;
                if (w[ROB_USED] > call.parts[i].owned) return call.failed(i, fail(tiles[i].h, PPP_ERR_HIP, "robust registration tiles: sums corrupt"));
                icp_row_terms(&call.part_rows[i], T, w);
                wsum += w[ROB_WSUM];
            }
            sc.weight_sum = (long long)wsum;
        }
        e = regt_merged(h0, call, T, rw); /* rw.pairs = used: what the step reads (B.104) */
        if (e) return e;
        if (rw.pairs > paired) return fail(h0, PPP_ERR_HIP, "robust registration tiles: sums corrupt");
        sc.used = rw.pairs;
        scales.push_back(sc);
        return (int)PPP_OK;
    });
    if (rc) return rc;
    const size_t last = (size_t)C.steps;
    /* B.109: the maps of the last evaluation -- its keys and residuals are the ones the tiles hold --, every tile's launch before any copy */
    for (size_t i = 0; i < count; ++i)
        if (wants_maps(i)) {
            rc = robt_enqueue_scatter(tiles[i], S.tune * scales[last].sigma, S.tune, scales[last].paired == 0);
            if (rc) return call.failed(i, rc);
        }
    for (size_t i = 0; i < count; ++i) {
        rc = trimt_copy_maps(tiles[i], map_of(status, i), map_of(weight, i), map_of(owned, i), cap);
        if (!rc) rc = robt_copy_residual(tiles[i], map_of(residual, i), cap);
        if (rc) return call.failed(i, rc);
    }
    std::vector<ppp_robust_registration_row> out(last + 1);
    for (size_t i = 0; i <= last; ++i) {
        ppp_robust_registration_row &o = out[i];
        memset(&o, 0, sizeof(o)); /* the padding too: rows compare as bytes */
        R[i].pairs = scales[i].paired; /* the step read `used` there */
        o.row = R[i];
        o.used = scales[i].used;
        o.weight_sum = scales[i].weight_sum;
        memcpy(&o.median_abs, &scales[i].tau, sizeof(float));
        o.sigma = scales[i].sigma;
    }
    if (stats) {
        stats->reg = registration_stats(R, C, call.whole.n, call.whole.owned, call.whole.shift, call.whole.centre, call.whole.length);
        auto rms = [](const ppp_robust_registration_row &r) { return r.weight_sum ? std::sqrt((double)r.row.E / (double)r.weight_sum) : (double)NAN; };
        stats->reg.rms_before = rms(out[0]); stats->reg.rms_after = rms(out[last]);
    }
    const size_t k = std::min(row_cap, last + 1);
    if (rows && k) memcpy(rows, out.data(), k * sizeof(ppp_robust_registration_row));
    return PPP_OK;
}

/* ---- the resident triangle mesh and the exact deviation against it (ppp_trimesh.h) ---- */
} // extern "C"

/* The mesh owns its buffers and a stream of its own: after ppp_trimesh_create it needs neither the handle nor any cloud. */
struct ppp_trimesh_s {
    int device = 0, num_cus = 1;
    hipStream_t stream = nullptr;
    DevBuf<TriRec> rec;
    DevBuf<unsigned> cell_start;
    DevBuf<int> cell_rec;
    TriGrid G = {};
    int n_tris = 0;
    /* the welded topology (ppp_trimesh_topology.h): built once, by the first call that needs it */
    /* ppp_trimesh_get_moments: the ten words, and the lock its callers take turns under */
    std::mutex mom_lock;
    DevBuf<unsigned long long> mom;
    std::mutex topo_lock;
    bool topo_built = false;
    ppp_trimesh_topology_stats topo_stats = {};
    TriTopo T = {};
    DevBuf<int> rec_of, vslot, eslot, table;
    DevBuf<unsigned char> eclass;
    DevBuf<unsigned> vbits;
    DevBuf<double> vpn, epn;
    ~ppp_trimesh_s() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace {
constexpr size_t TRIMESH_MAX = 0x7fffffffu / 8; /* triangles and vertices: ppp_set_cloud_mesh's limit */

/* the grid's dimensions for this cell; false: more than TM_MAX_CELLS cells */
static bool trimesh_dims(const double *mn, const double *mx, double cell, int *dim)
{
    double cells = 1.0;
    for (int d = 0; d < 3; ++d) {
        const double c = std::floor((mx[d] - mn[d]) / cell) + 1.0; /* tm_cell of the upper corner, + 1 */
        if (!(c <= (double)TM_MAX_CELLS)) return false;
        dim[d] = (int)c;
        cells *= c;
    }
    return cells <= (double)TM_MAX_CELLS;
}

static TmOut trimesh_outputs(double *distance, double *closest, double *deviation, long long *fix, float *d2f, int *tri_index, unsigned char *region,
                             unsigned char *status)
{
    TmOut O;
    O.distance = distance; O.closest = closest; O.deviation = deviation; O.fix = fix; O.d2f = d2f; O.tri_index = tri_index; O.region = region; O.status = status;
    return O;
}
} // namespace

extern "C" {

void ppp_default_trimesh_params(ppp_trimesh_params *tp)
{
    if (!tp) return;
    tp->cell = 0.f; tp->orient = PPP_TRIMESH_WINDING;
}

void ppp_trimesh_destroy(ppp_trimesh m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

int ppp_trimesh_create(ppp_handle h, const float *verts, size_t n_verts, const int *tris, size_t n_tris, const ppp_trimesh_params *tp,
                       const float *viewpoint, ppp_trimesh *out, ppp_trimesh_stats *stats)
{
    if (out) *out = nullptr;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!h) return PPP_ERR_ARG;
    if (!out) return fail(h, PPP_ERR_ARG, "trimesh: out is NULL");
    if (!verts || !tp) return fail(h, PPP_ERR_ARG, "trimesh: vertices and parameters are required");
    const bool automatic = tp->cell == 0.f;
    if (!automatic && (!(tp->cell > 0.f) || !std::isfinite(tp->cell))) return fail(h, PPP_ERR_ARG, "trimesh: cell must be 0 (automatic) or positive and finite");
    if (tp->orient != PPP_TRIMESH_WINDING && tp->orient != PPP_TRIMESH_VIEWPOINT) return fail(h, PPP_ERR_ARG, "trimesh: orient is PPP_TRIMESH_WINDING or PPP_TRIMESH_VIEWPOINT");
    if (n_tris == 0) return fail(h, PPP_ERR_ARG, "trimesh: no triangle");
    if (!tris && (n_verts % 3 || n_verts / 3 != n_tris)) return fail(h, PPP_ERR_ARG, "trimesh: a soup (tris == NULL) has three vertices per triangle");
    if (n_tris > TRIMESH_MAX || n_verts > TRIMESH_MAX) return fail(h, PPP_ERR_CAPACITY, "trimesh: mesh too large");
    HIPCHK(h, hipSetDevice(h->device));
    std::unique_ptr<ppp_trimesh_s> m(new ppp_trimesh_s);
    m->device = h->device; m->num_cus = h->num_cus;
    ppp_trimesh_stats st = {};
    st.triangles = n_tris;
    DevBuf<char> raw, tmp;
    DevBuf<float> V;
    DevBuf<int> T, val;
    DevBuf<unsigned> valid, rank, cnt, off, key, key_sorted, words;
    DevBuf<unsigned long long> side_sum;
    const size_t nv = std::max<size_t>(n_verts, 1);
    HIPCHK(h, raw.ensure(12 * nv)); HIPCHK(h, V.ensure(3 * nv)); HIPCHK(h, valid.ensure(n_tris + 1)); HIPCHK(h, rank.ensure(n_tris + 1));
    HIPCHK(h, words.ensure(8)); HIPCHK(h, side_sum.ensure(1));
    if (tris) HIPCHK(h, T.ensure(3 * n_tris));
    /* the vertices become resident ones by the conversion of every cloud (k_ingest), as ppp_set_cloud_mesh's do */
    if (n_verts) {
        HIPCHK(h, hipMemcpyAsync(raw.p, verts, 12 * n_verts, hipMemcpyHostToDevice, h->stream));
#ifdef PPP_KERNELS_FOREIGN /* (the engine's kernel, instantiated here: ppp_kernels.h) */
        LAUNCH(h, "k_ingest", k_ingest<>, (unsigned)((n_verts + 255) / 256), 256, 0, raw.p, (size_t)12, (int)n_verts, h->P.change_range, V.p, V.p + nv, V.p + 2 * nv);
#else
        LAUNCH(h, "k_ingest", k_ingest, (unsigned)((n_verts + 255) / 256), 256, 0, raw.p, (size_t)12, (int)n_verts, h->P.change_range, V.p, V.p + nv, V.p + 2 * nv);
#endif
    }
    if (tris) HIPCHK(h, hipMemcpyAsync(T.p, tris, 12 * n_tris, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(words.p, 0, 8 * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(side_sum.p, 0, sizeof(unsigned long long), h->stream));
    MeshArgs A;
    A.Vx = V.p; A.Vy = V.p + nv; A.Vz = V.p + 2 * nv; A.n_verts = (int)n_verts;
    A.tris = tris ? T.p : nullptr; A.n_tris = (int)n_tris;
    A.pitch = 0.0; A.front = 0;
    for (int d = 0; d < 3; ++d) A.vp[d] = viewpoint ? (double)viewpoint[d] : 0.0;
    LAUNCH(h, "k_tm_bounds", k_tm_bounds, (unsigned)((n_tris + 1 + TM_T - 1) / TM_T), TM_T, 0, A, valid.p, words.p);
    int rc = scan_exclusive(h, "trimesh_scan_rank", tmp, valid.p, rank.p, n_tris + 1);
    if (rc) return rc;
    unsigned bb[6] = {0, 0, 0, 0, 0, 0}, indexed = 0;
    HIPCHK(h, hipMemcpyAsync(bb, words.p, sizeof(bb), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&indexed, rank.p + n_tris, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (indexed > n_tris) return fail(h, PPP_ERR_HIP, "trimesh: counts corrupt");
    st.indexed = indexed; st.degenerate = n_tris - indexed;
    if (stats) *stats = st;
    if (indexed == 0) return fail(h, PPP_ERR_ARG, "trimesh: nothing to index: every triangle is degenerate");
    TriGrid &G = m->G;
    double extent = 0.0;
    for (int d = 0; d < 3; ++d) {
        st.mn[d] = ordered_unkey(~bb[d]); st.mx[d] = ordered_unkey(bb[3 + d]);
        G.mn[d] = (double)st.mn[d]; G.mx[d] = (double)st.mx[d];
        G.vp[d] = A.vp[d];
        extent = std::max(extent, G.mx[d] - G.mn[d]);
    }
    if (!(extent > 0.0) || !std::isfinite(extent)) return fail(h, PPP_ERR_HIP, "trimesh: bounds corrupt");
    G.by_viewpoint = tp->orient == PPP_TRIMESH_VIEWPOINT;
    G.indexed = (int)indexed;
    HIPCHK(h, m->rec.ensure(indexed));
    G.rec = m->rec.p;
    LAUNCH(h, "k_tm_records", k_tm_records, (unsigned)((n_tris + TM_T - 1) / TM_T), TM_T, 0, A, rank.p, m->rec.p);
    const unsigned grec = (unsigned)(((size_t)indexed + 1 + TM_T - 1) / TM_T);
    float cell = tp->cell;
    if (automatic) { /* the mean longest box side of the indexed triangles (an integer sum: the same in every run) */
        LAUNCH(h, "k_tm_sides", k_tm_sides, grec, TM_T, 0, G, extent, side_sum.p);
        unsigned long long sum = 0;
        HIPCHK(h, copy_sync(h, &sum, side_sum.p, sizeof(sum), hipMemcpyDeviceToHost));
        cell = (float)((double)sum / (double)indexed / TM_SIDE_SCALE * extent);
        if (!(cell > 0.f) || !std::isfinite(cell)) cell = (float)extent;
        if (!(cell > 0.f) || !std::isfinite(cell)) return fail(h, PPP_ERR_ARG, "trimesh: no cell for this mesh's extent");
    }
    HIPCHK(h, cnt.ensure((size_t)indexed + 1)); HIPCHK(h, off.ensure((size_t)indexed + 1));
    unsigned pairs = 0;
    for (;;) { /* an automatic cell doubles until the grid and the pair list fit; a given one is refused */
        G.cell = (double)cell;
        bool fits = std::isfinite(cell) && trimesh_dims(G.mn, G.mx, G.cell, G.dim);
        if (!fits && !automatic) return fail(h, PPP_ERR_CAPACITY, "trimesh: this cell makes more than 2^24 cells");
        if (fits) {
            LAUNCH(h, "k_tm_count", k_tm_count, grec, TM_T, 0, G, cnt.p);
            rc = scan_exclusive(h, "trimesh_scan_pairs", tmp, cnt.p, off.p, (size_t)indexed + 1);
            if (rc) return rc;
            HIPCHK(h, copy_sync(h, &pairs, off.p + indexed, sizeof(unsigned), hipMemcpyDeviceToHost));
            fits = pairs <= TM_MAX_PAIRS;
            if (!fits && !automatic) return fail(h, PPP_ERR_CAPACITY, "trimesh: this cell makes 2^31 - 1 (triangle, cell) pairs or more");
        }
        if (fits) break;
        if (!std::isfinite(cell)) return fail(h, PPP_ERR_CAPACITY, "trimesh: no cell fits this mesh");
        cell *= 2.f;
    }
    if (pairs < indexed) return fail(h, PPP_ERR_HIP, "trimesh: pair count corrupt");
    const size_t cells = (size_t)G.dim[0] * (size_t)G.dim[1] * (size_t)G.dim[2];
    HIPCHK(h, key.ensure(pairs)); HIPCHK(h, key_sorted.ensure(pairs)); HIPCHK(h, val.ensure(pairs));
    HIPCHK(h, m->cell_rec.ensure(pairs)); HIPCHK(h, m->cell_start.ensure(cells + 1));
    LAUNCH(h, "k_tm_pairs", k_tm_pairs, (unsigned)(((size_t)pairs + TM_T - 1) / TM_T), TM_T, 0, G, off.p, pairs, key.p, val.p);
    {
        int end_bit = 1;
        while (end_bit < 32 && (cells - 1) >> end_bit) ++end_bit;
        size_t bytes = 0;
        HIPCHK(h, ppp_sort_pairs_u32(nullptr, &bytes, key.p, key_sorted.p, val.p, m->cell_rec.p, pairs, end_bit, h->stream));
        HIPCHK(h, tmp.ensure(bytes));
        KTimer *t = h->timing ? timer_for(h, "trimesh_sort_pairs") : nullptr;
        if (t) (void)hipEventRecord(t->e0[t->used], h->stream);
        const hipError_t e = ppp_sort_pairs_u32(tmp.p, &bytes, key.p, key_sorted.p, val.p, m->cell_rec.p, pairs, end_bit, h->stream);
        if (t) { (void)hipEventRecord(t->e1[t->used], h->stream); t->used++; }
        HIPCHK(h, e);
    }
    LAUNCH(h, "k_tm_cell_start", k_tm_cell_start, (unsigned)((cells + 1 + TM_T - 1) / TM_T), TM_T, 0, key_sorted.p, pairs, (unsigned)cells, m->cell_start.p);
    HIPCHK(h, hipMemsetAsync(words.p, 0, sizeof(unsigned), h->stream));
    LAUNCH(h, "k_tm_max_per_cell", k_tm_max_per_cell, (unsigned)((cells + TM_T - 1) / TM_T), TM_T, 0, m->cell_start.p, (unsigned)cells, words.p);
    unsigned most = 0;
    HIPCHK(h, copy_sync(h, &most, words.p, sizeof(unsigned), hipMemcpyDeviceToHost)); /* the wait: the scratch may go */
    G.cell_start = m->cell_start.p; G.cell_rec = m->cell_rec.p;
    HIPCHK(h, hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    for (int d = 0; d < 3; ++d) st.cells[d] = (size_t)G.dim[d];
    st.pairs = pairs; st.max_per_cell = most; st.cell = cell;
    m->n_tris = (int)n_tris;
    if (stats) *stats = st;
    *out = m.release();
    return PPP_OK;
}

int ppp_trimesh_create_stl(ppp_handle h, const char *path, const ppp_trimesh_params *tp, const float *viewpoint, ppp_trimesh *out, ppp_trimesh_stats *stats)
{
    if (out) *out = nullptr;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!h) return PPP_ERR_ARG;
    if (!path) return fail(h, PPP_ERR_ARG, "trimesh: no file name");
    float *v9 = nullptr;
    size_t nt = 0;
    int rc = ppp_load_stl(path, &v9, &nt);
    if (rc != PPP_OK) return fail(h, rc, std::string("not a readable STL file: ") + path);
    rc = ppp_trimesh_create(h, v9, 3 * nt, nullptr, nt, tp, viewpoint, out, stats);
    ppp_free(v9);
    return rc;
}

/* The welded topology of m (ppp_trimesh_topology.h), built once under the mesh's lock on the mesh's stream: the
   corner keys, three stable passes, the vertex runs; the half-edge pairs, two stable passes, the edge runs; the table and the
   vertex counts; one wait.  h (may be NULL): a handle whose kernel timers, where they are on, bracket each step. */
static int trimesh_topology_build(ppp_trimesh m, ppp_handle h)
{
    std::lock_guard<std::mutex> lock(m->topo_lock);
    if (m->topo_built) return PPP_OK;
#define TT_CHK(expr) do { if ((expr) != hipSuccess) return PPP_ERR_HIP; } while (0)
    TT_CHK(hipSetDevice(m->device));
    const size_t R = (size_t)m->G.indexed, S = 3 * R;
    const int slots = (int)S;
    const unsigned grid = (unsigned)((S + TT_T - 1) / TT_T);
    DevBuf<unsigned> kx, ky, kz, ka, kb;
    DevBuf<int> va, vb;
    DevBuf<unsigned char> up;
    DevBuf<unsigned long long> cnt;
    DevBuf<char> tmp;
    TT_CHK(kx.ensure(S)); TT_CHK(ky.ensure(S)); TT_CHK(kz.ensure(S)); TT_CHK(ka.ensure(S)); TT_CHK(kb.ensure(S));
    TT_CHK(va.ensure(S)); TT_CHK(vb.ensure(S)); TT_CHK(up.ensure(S)); TT_CHK(cnt.ensure(TT_WORDS));
    TT_CHK(m->rec_of.ensure((size_t)m->n_tris)); TT_CHK(m->vslot.ensure(S)); TT_CHK(m->eslot.ensure(S)); TT_CHK(m->table.ensure(6 * R));
    TT_CHK(m->eclass.ensure(S)); TT_CHK(m->vbits.ensure(S)); TT_CHK(m->vpn.ensure(3 * S)); TT_CHK(m->epn.ensure(3 * S));
    TT_CHK(hipMemsetAsync(m->rec_of.p, 0xff, (size_t)m->n_tris * sizeof(int), m->stream)); /* -1: degenerate */
    TT_CHK(hipMemsetAsync(m->vbits.p, 0, S * sizeof(unsigned), m->stream));
    TT_CHK(hipMemsetAsync(m->eclass.p, 0xff, S, m->stream));
    TT_CHK(hipMemsetAsync(cnt.p, 0, TT_WORDS * sizeof(unsigned long long), m->stream));
    auto timed = [&](const char *name, auto &&step) -> hipError_t {
        KTimer *t = h && h->timing ? timer_for(h, name) : nullptr;
        if (t) (void)hipEventRecord(t->e0[t->used], m->stream);
        (void)hipGetLastError();
        hipError_t e = step();
        if (e == hipSuccess) e = hipGetLastError();
        if (t) { (void)hipEventRecord(t->e1[t->used], m->stream); t->used++; }
        return e;
    };
#define TT_LAUNCH(name, kern, ...) TT_CHK(timed(name, [&]() { hipLaunchKernelGGL(kern, dim3(grid), dim3(TT_T), 0, m->stream, __VA_ARGS__); return hipSuccess; }))
    auto sort = [&](const unsigned *key_in, const int *val_in, int *val_out, int end_bit) -> hipError_t {
        size_t bytes = 0;
        hipError_t e = ppp_sort_pairs_u32(nullptr, &bytes, key_in, ka.p, val_in, val_out, S, end_bit, m->stream);
        if (e == hipSuccess) e = tmp.ensure(bytes);
        if (e != hipSuccess) return e;
        return timed("trimesh_topology_sort", [&]() { return ppp_sort_pairs_u32(tmp.p, &bytes, key_in, ka.p, val_in, val_out, S, end_bit, m->stream); });
    };
    const TriRec *rec = m->rec.p;
    TT_LAUNCH("k_tt_corners", k_tt_corners, rec, slots, kx.p, ky.p, kz.p, va.p, m->rec_of.p);
    TT_CHK(sort(kz.p, va.p, vb.p, 32));
    TT_LAUNCH("k_tt_gather", k_tt_gather, slots, (const unsigned *)ky.p, (const int *)vb.p, kb.p);
    TT_CHK(sort(kb.p, vb.p, va.p, 32));
    TT_LAUNCH("k_tt_gather", k_tt_gather, slots, (const unsigned *)kx.p, (const int *)va.p, kb.p);
    TT_CHK(sort(kb.p, va.p, vb.p, 32));
    TT_LAUNCH("k_tt_vertices", k_tt_vertices, m->G, slots, (const int *)vb.p, (const unsigned *)kx.p, (const unsigned *)ky.p, (const unsigned *)kz.p, m->vslot.p,
              m->vpn.p, cnt.p);
    int id_bits = 1;
    while (id_bits < 32 && (S - 1) >> id_bits) ++id_bits;
    TT_LAUNCH("k_tt_halfedges", k_tt_halfedges, m->G, slots, (const int *)m->vslot.p, kx.p, ky.p, up.p, va.p); /* kx: the smaller id, ky: the larger */
    TT_CHK(sort(ky.p, va.p, vb.p, id_bits));
    TT_LAUNCH("k_tt_gather", k_tt_gather, slots, (const unsigned *)kx.p, (const int *)vb.p, kb.p);
    TT_CHK(sort(kb.p, vb.p, va.p, id_bits));
    TT_LAUNCH("k_tt_edges", k_tt_edges, m->G, slots, (const int *)va.p, (const unsigned *)kx.p, (const unsigned *)ky.p, (const unsigned char *)up.p, m->eslot.p,
              m->eclass.p, m->epn.p, m->vbits.p, cnt.p);
    TT_LAUNCH("k_tt_table", k_tt_table, rec, slots, (const int *)m->vslot.p, (const int *)m->eslot.p, (const unsigned *)m->vbits.p, m->table.p, cnt.p);
#undef TT_LAUNCH
    unsigned long long c[TT_WORDS];
    TT_CHK(hipMemcpyAsync(c, cnt.p, sizeof(c), hipMemcpyDeviceToHost, m->stream));
    TT_CHK(hipStreamSynchronize(m->stream)); /* the wait: the scratch may go */
#undef TT_CHK
    if (c[0] == 0 || c[0] > S || c[1] == 0 || c[1] > S || c[2] + c[3] + c[4] + c[5] != c[1] || c[6] > c[0] || c[7] > c[0]) return PPP_ERR_HIP;
    ppp_trimesh_topology_stats &st = m->topo_stats;
    st.vertices = (size_t)c[0]; st.edges = (size_t)c[1]; st.border_edges = (size_t)c[2]; st.manifold_edges = (size_t)c[3];
    st.inconsistent_edges = (size_t)c[4]; st.nonmanifold_edges = (size_t)c[5]; st.border_vertices = (size_t)c[6]; st.irregular_vertices = (size_t)c[7];
    st.closed = c[2] == 0 && c[4] == 0 && c[5] == 0;
    TriTopo &T = m->T;
    T.rec_of = m->rec_of.p; T.vslot = m->vslot.p; T.eslot = m->eslot.p; T.eclass = m->eclass.p; T.vbits = m->vbits.p; T.vpn = m->vpn.p; T.epn = m->epn.p;
    T.table = m->table.p; T.n_tris = m->n_tris;
    m->topo_built = true;
    return PPP_OK;
}

int ppp_trimesh_topology(ppp_trimesh m, ppp_trimesh_topology_stats *stats)
{
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!m) return PPP_ERR_ARG;
    const int rc = trimesh_topology_build(m, nullptr);
    if (rc == PPP_OK && stats) *stats = m->topo_stats;
    return rc;
}

int ppp_trimesh_get_topology(ppp_trimesh m, int *vertex_id, int *edge_id, unsigned char *edge_class, unsigned char *vertex_bits, double *vertex_normal,
                             double *edge_normal, size_t cap, ppp_trimesh_topology_stats *stats)
{
    const int rc = ppp_trimesh_topology(m, stats);
    if (rc) return rc;
    const size_t k = std::min(cap, (size_t)m->n_tris);
    if (k == 0 || !(vertex_id || edge_id || edge_class || vertex_bits || vertex_normal || edge_normal)) return PPP_OK;
#define TM_CHK(expr) do { if ((expr) != hipSuccess) return PPP_ERR_HIP; } while (0)
    TM_CHK(hipSetDevice(m->device));
    DevBuf<int> d_v, d_e;
    DevBuf<unsigned char> d_c, d_b;
    DevBuf<double> d_vn, d_en;
    TM_CHK(d_v.ensure(3 * k)); TM_CHK(d_e.ensure(3 * k)); TM_CHK(d_c.ensure(3 * k)); TM_CHK(d_b.ensure(3 * k)); TM_CHK(d_vn.ensure(9 * k)); TM_CHK(d_en.ensure(9 * k));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tt_export, dim3((unsigned)((k + TT_T - 1) / TT_T)), dim3(TT_T), 0, m->stream, (const TriRec *)m->rec.p, m->T, (int)k, d_v.p, d_e.p, d_c.p, d_b.p,
                       d_vn.p, d_en.p);
    TM_CHK(hipGetLastError());
    if (vertex_id) TM_CHK(hipMemcpyAsync(vertex_id, d_v.p, 3 * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (edge_id) TM_CHK(hipMemcpyAsync(edge_id, d_e.p, 3 * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (edge_class) TM_CHK(hipMemcpyAsync(edge_class, d_c.p, 3 * k, hipMemcpyDeviceToHost, m->stream));
    if (vertex_bits) TM_CHK(hipMemcpyAsync(vertex_bits, d_b.p, 3 * k, hipMemcpyDeviceToHost, m->stream));
    if (vertex_normal) TM_CHK(hipMemcpyAsync(vertex_normal, d_vn.p, 9 * k * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    if (edge_normal) TM_CHK(hipMemcpyAsync(edge_normal, d_en.p, 9 * k * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    TM_CHK(hipStreamSynchronize(m->stream));
#undef TM_CHK
    return PPP_OK;
}

/* The primitive: the caller's points up, k_mesh_nearest on the mesh's own stream, the maps down.  No handle: an error is its
   code.  sign: ppp_trimesh_signed_nearest's four maps -- the topology where it is missing, and k_mesh_sign behind the search. */
struct TrimeshSignMaps { double *signed_distance, *pseudonormal; unsigned char *feature, *flags; };
static int trimesh_nearest(ppp_trimesh m, const float *xyz, size_t n, float max_dist, const TrimeshSignMaps *sign, double *distance, double *closest,
                           double *deviation, int *tri_index, unsigned char *region, unsigned char *status)
{
    if (!m || (!xyz && n) || !(max_dist > 0.f)) return PPP_ERR_ARG;
    if (n > 0x7fffffffu / 8) return PPP_ERR_CAPACITY;
    if (sign) { const int rc = trimesh_topology_build(m, nullptr); if (rc) return rc; }
    if (n == 0) return PPP_OK;
#define TM_CHK(expr) do { if ((expr) != hipSuccess) return PPP_ERR_HIP; } while (0)
    TM_CHK(hipSetDevice(m->device));
    DevBuf<float> q;
    DevBuf<double> d_dist, d_close, d_dev, d_signed, d_pn;
    DevBuf<int> d_tri;
    DevBuf<unsigned char> d_region, d_status, d_feature, d_flags;
    TM_CHK(q.ensure(3 * n)); TM_CHK(d_status.ensure(n));
    if (distance) TM_CHK(d_dist.ensure(n));
    if (closest) TM_CHK(d_close.ensure(3 * n));
    if (deviation) TM_CHK(d_dev.ensure(n));
    if (tri_index || sign) TM_CHK(d_tri.ensure(n));
    if (region) TM_CHK(d_region.ensure(n));
    if (sign) {
        TM_CHK(d_signed.ensure(n));
        if (sign->pseudonormal) TM_CHK(d_pn.ensure(3 * n));
        if (sign->feature) TM_CHK(d_feature.ensure(n));
        if (sign->flags) TM_CHK(d_flags.ensure(n));
    }
    TM_CHK(hipMemcpyAsync(q.p, xyz, 12 * n, hipMemcpyHostToDevice, m->stream));
    const double md2 = (double)max_dist * (double)max_dist;
    const TmOut O = trimesh_outputs(d_dist.p, d_close.p, d_dev.p, nullptr, nullptr, d_tri.p, d_region.p, d_status.p);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mesh_nearest, dim3((unsigned)((n + TM_T - 1) / TM_T)), dim3(TM_T), 0, m->stream, (const float4 *)nullptr, (const float *)q.p, (int)n, m->G,
                       md2, O);
    TM_CHK(hipGetLastError());
    if (sign) {
        TmSignOut SO;
        SO.signed_distance = d_signed.p; SO.pseudonormal = d_pn.p; SO.dev = nullptr; SO.fix = nullptr; SO.feature = d_feature.p; SO.flags = d_flags.p;
        SO.tri_index = d_tri.p; SO.status = d_status.p;
        hipLaunchKernelGGL(k_mesh_sign, dim3((unsigned)((n + TM_T - 1) / TM_T)), dim3(TM_T), 0, m->stream, (const float4 *)nullptr, (const float *)q.p, (int)n, m->G,
                           m->T, SO);
        TM_CHK(hipGetLastError());
        if (sign->signed_distance) TM_CHK(hipMemcpyAsync(sign->signed_distance, d_signed.p, n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (sign->pseudonormal) TM_CHK(hipMemcpyAsync(sign->pseudonormal, d_pn.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (sign->feature) TM_CHK(hipMemcpyAsync(sign->feature, d_feature.p, n, hipMemcpyDeviceToHost, m->stream));
        if (sign->flags) TM_CHK(hipMemcpyAsync(sign->flags, d_flags.p, n, hipMemcpyDeviceToHost, m->stream));
    }
    if (distance) TM_CHK(hipMemcpyAsync(distance, d_dist.p, n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    if (closest) TM_CHK(hipMemcpyAsync(closest, d_close.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    if (deviation) TM_CHK(hipMemcpyAsync(deviation, d_dev.p, n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    if (tri_index) TM_CHK(hipMemcpyAsync(tri_index, d_tri.p, n * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (region) TM_CHK(hipMemcpyAsync(region, d_region.p, n, hipMemcpyDeviceToHost, m->stream));
    if (status) TM_CHK(hipMemcpyAsync(status, d_status.p, n, hipMemcpyDeviceToHost, m->stream));
    TM_CHK(hipStreamSynchronize(m->stream));
#undef TM_CHK
    return PPP_OK;
}

int ppp_trimesh_nearest(ppp_trimesh m, const float *xyz, size_t n, float max_dist, double *distance, double *closest, double *deviation, int *tri_index,
                        unsigned char *region, unsigned char *status)
{
    return trimesh_nearest(m, xyz, n, max_dist, nullptr, distance, closest, deviation, tri_index, region, status);
}

int ppp_trimesh_signed_nearest(ppp_trimesh m, const float *xyz, size_t n, float max_dist, double *signed_distance, double *pseudonormal, unsigned char *feature,
                               unsigned char *flags, double *distance, double *closest, double *deviation, int *tri_index, unsigned char *region,
                               unsigned char *status)
{
    const TrimeshSignMaps sign = {signed_distance, pseudonormal, feature, flags};
    return trimesh_nearest(m, xyz, n, max_dist, &sign, distance, closest, deviation, tri_index, region, status);
}

/* The exact deviation map: the scan's slab index, k_tm_fill and k_mesh_nearest over its points in slab order,
   then ppp_get_deviation's own tail (deviation_tail) and the counts by region, all on the scan's stream; one wait. */
struct MeshSignMaps { unsigned char *feature, *flags; ppp_mesh_signed_deviation_stats *stats; };
static int mesh_deviation(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp, const MeshSignMaps *sign, double *deviation, double *smoothed,
                          double *distance, int *tri_index, unsigned char *region, unsigned char *status, double *target, size_t cap,
                          ppp_mesh_deviation_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const std::string w = sign ? "mesh signed deviation" : "mesh deviation";
    if (!m || !dp) return fail(h, PPP_ERR_ARG, w + ": no mesh or no parameters");
    int rc = deviation_params_ok(h, *dp, w, nullptr);
    if (rc) return rc;
    if (m->device != h->device) return fail(h, PPP_ERR_ARG, w + ": the mesh is on another device than the handle");
    const ppp_deviation_params P = *dp;
    const bool smooth = P.smooth_radius > 0.f;
    rc = deviation_side(h, h, "the scan", w.c_str());
    if (rc) return rc;
    const size_t N = h->n;
    if (deviation_sum_overflows(P, N)) return fail(h, PPP_ERR_ARG, w + ": max_dist 2^24 n reaches 2^62: the smoothing's integer sum could overflow");
    if (sign) { /* the topology on the mesh's stream, waited for: read-only from here on */
        rc = trimesh_topology_build(m, h);
        if (rc) return fail(h, rc, w + ": the mesh's topology could not be built");
        HIPCHK(h, hipSetDevice(h->device));
    }
    auto &D = h->deviation;
    const size_t N1 = std::max<size_t>(N, 1);
    const MapParts parts(h, N);
    const int nq = h->hmeta.n_sorted;
    HIPCHK(h, D.dev.ensure(N1)); HIPCHK(h, D.target.ensure(N1)); HIPCHK(h, D.fix.ensure(N1)); HIPCHK(h, D.d2.ensure(N1)); HIPCHK(h, D.dist.ensure(N1));
    HIPCHK(h, D.ref_index.ensure(N1)); HIPCHK(h, D.status.ensure(N1)); HIPCHK(h, D.region.ensure(N1)); HIPCHK(h, D.acc.ensure(DEV_ACC_WORDS));
    HIPCHK(h, D.psum.ensure(2 * (size_t)parts.grid)); HIPCHK(h, D.macc.ensure(4));
    if (smooth) HIPCHK(h, D.smoothed.ensure(N1));
    HIPCHK(h, hipMemsetAsync(D.acc.p, 0, DEV_ACC_WORDS * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(D.macc.p, 0, 4 * sizeof(unsigned long long), h->stream));
    const unsigned gn = (unsigned)std::min<size_t>((N1 + TM_T - 1) / TM_T, 2 * (size_t)h->num_cus);
    LAUNCH(h, "k_tm_fill", k_tm_fill, gn, TM_T, 0, (int)N, D.dist.p, D.ref_index.p, D.region.p, D.status.p); /* points outside the index: not finite */
    if (nq > 0) {
        const TmOut O = trimesh_outputs(D.dist.p, nullptr, D.dev.p, D.fix.p, D.d2.p, D.ref_index.p, D.region.p, D.status.p);
        LAUNCH(h, "k_mesh_nearest", k_mesh_nearest, (unsigned)((nq + TM_T - 1) / TM_T), TM_T, 0, (const float4 *)h->sorted4.p, (const float *)nullptr, nq, m->G,
               (double)P.max_dist * (double)P.max_dist, O);
    }
    LAUNCH(h, "k_tm_region_stats", k_tm_region_stats, gn, TM_T, 0, (int)N, D.status.p, D.region.p, D.dist.p, D.macc.p);
    if (sign) { /* the signed distance takes the deviation's place, in the map and in its fixed-point term, before the tail reads them */
        HIPCHK(h, D.feature.ensure(N1)); HIPCHK(h, D.flags.ensure(N1)); HIPCHK(h, D.sacc.ensure(5));
        HIPCHK(h, hipMemsetAsync(D.sacc.p, 0, 5 * sizeof(unsigned long long), h->stream));
        LAUNCH(h, "k_tm_sign_fill", k_tm_sign_fill, gn, TM_T, 0, (int)N, D.feature.p, D.flags.p);
        if (nq > 0) {
            TmSignOut SO;
            SO.signed_distance = D.dev.p; SO.pseudonormal = nullptr; SO.dev = nullptr; SO.fix = D.fix.p; SO.feature = D.feature.p; SO.flags = D.flags.p;
            SO.tri_index = D.ref_index.p; SO.status = D.status.p;
            LAUNCH(h, "k_mesh_sign", k_mesh_sign, (unsigned)((nq + TM_T - 1) / TM_T), TM_T, 0, (const float4 *)h->sorted4.p, (const float *)nullptr, nq, m->G, m->T, SO);
        }
        LAUNCH(h, "k_tm_sign_stats", k_tm_sign_stats, gn, TM_T, 0, (int)N, D.status.p, D.flags.p, D.dev.p, D.sacc.p);
    }
    const double *v = nullptr;
    ppp_mesh_deviation_stats st = {};
    rc = deviation_tail(h, P, parts, w.c_str(), &st.dev, &v);
    if (rc) return rc;
    unsigned long long macc[4];
    HIPCHK(h, copy_sync(h, macc, D.macc.p, sizeof(macc), hipMemcpyDeviceToHost));
    if (macc[0] + macc[1] + macc[2] != st.dev.matched) return fail(h, PPP_ERR_HIP, w + ": statistics corrupt");
    st.on_face = (size_t)macc[0]; st.on_edge = (size_t)macc[1]; st.on_vertex = (size_t)macc[2];
    st.max_distance = (double)NAN;
    if (st.dev.matched) memcpy(&st.max_distance, &macc[3], sizeof(double));
    if (stats) *stats = st;
    const size_t k = std::min(cap, N);
    rc = deviation_copy_out(h, k, v, deviation, smoothed, tri_index, status, target);
    if (rc) return rc;
    if (distance && k) HIPCHK(h, copy_sync(h, distance, D.dist.p, k * sizeof(double), hipMemcpyDeviceToHost));
    if (region && k) HIPCHK(h, copy_sync(h, region, D.region.p, k, hipMemcpyDeviceToHost));
    if (sign) {
        unsigned long long sacc[5];
        HIPCHK(h, copy_sync(h, sacc, D.sacc.p, sizeof(sacc), hipMemcpyDeviceToHost));
        if (sacc[3] + sacc[4] > st.dev.matched) return fail(h, PPP_ERR_HIP, w + ": statistics corrupt");
        if (sign->stats) {
            ppp_mesh_signed_deviation_stats &ss = *sign->stats;
            ss.mesh = st;
            ss.on_border = (size_t)sacc[0]; ss.irregular = (size_t)sacc[1]; ss.fallback = (size_t)sacc[2]; ss.negative = (size_t)sacc[3]; ss.positive = (size_t)sacc[4];
        }
        if (sign->feature && k) HIPCHK(h, copy_sync(h, sign->feature, D.feature.p, k, hipMemcpyDeviceToHost));
        if (sign->flags && k) HIPCHK(h, copy_sync(h, sign->flags, D.flags.p, k, hipMemcpyDeviceToHost));
    }
    return PPP_OK;
}

int ppp_get_mesh_deviation(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp, double *deviation, double *smoothed, double *distance, int *tri_index,
                           unsigned char *region, unsigned char *status, double *target, size_t cap, ppp_mesh_deviation_stats *stats)
{
    return mesh_deviation(h, m, dp, nullptr, deviation, smoothed, distance, tri_index, region, status, target, cap, stats);
}

/* The signed deviation map: ppp_get_mesh_deviation's launches with k_mesh_sign (and the fill and the counts of
   its two maps) between the search and the tail. */
int ppp_get_mesh_signed_deviation(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp, double *signed_distance, double *smoothed, double *distance,
                                  int *tri_index, unsigned char *region, unsigned char *feature, unsigned char *flags, unsigned char *status, double *target,
                                  size_t cap, ppp_mesh_signed_deviation_stats *stats)
{
    const MeshSignMaps sign = {feature, flags, stats};
    return mesh_deviation(h, m, dp, &sign, signed_distance, smoothed, distance, tri_index, region, status, target, cap, nullptr);
}

/* What a chain against the mesh needs before its first launch (w: the call's name): the mesh on the handle's device, the
   scan's slab index, ppp_register's shift (B.68), and the rest of F from the mesh's box (B.126). */
static void mesh_box_floats(const TriGrid &M, float *mn, float *mx)
{
    for (int d = 0; d < 3; ++d) { mn[d] = (float)M.mn[d]; mx[d] = (float)M.mx[d]; } /* (floats, widened: exact) */
}

static int mesh_registration_setup(ppp_handle h, ppp_trimesh m, const char *w, const ppp_registration_params &P, IcpFrame &F, int &shift)
{
    if (m->device != h->device) return fail(h, PPP_ERR_ARG, std::string(w) + ": the mesh is on another device than the handle");
    const int rc = deviation_side(h, h, "the scan", w);
    if (rc) return rc;
    shift = icp_shift(h->n, F.md2);
    if (shift < 16) return fail(h, PPP_ERR_ARG, std::string(w) + ": fewer than 16 fractional bits are left (n max_dist^2 too large): the integer sums could overflow");
    float mn[3], mx[3];
    mesh_box_floats(m->G, mn, mx);
    frame_from_bounds(mn, mx, (double)P.max_dist, shift, F.c, &F.Ln, &F.scale);
    return PPP_OK;
}

/* The mesh registration chain: registration_chain's shape with the mesh in the reference's place -- the scan's
   slab index, then iterations + 1 evaluations (k_mesh_reg_search and k_mesh_reg_sum; k_mesh_reg_terms in a fused build) and iterations steps (k_reg_step, unchanged) back to back on the
   scan's stream, in h->registration's buffers, and one wait.  The mesh is read-only since its create call waited: nothing to
   wait for on its side.  !loop: the one evaluation of ppp_get_mesh_registration_terms. */
static int mesh_registration_chain(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T0, bool loop,
                                   ppp_registration_row *rows, size_t row_cap, ppp_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!m || !rp) return fail(h, PPP_ERR_ARG, "mesh registration: no mesh or no parameters");
    if (!rows && row_cap) return fail(h, PPP_ERR_ARG, "mesh registration: rows is NULL with row_cap > 0");
    const ppp_registration_params P = *rp;
    IcpFrame F;
    int rc = registration_params_ok(h, P, F);
    if (rc) return rc;
    const int iterations = loop ? P.iterations : 0;
    double T[12];
    rc = opening_transform(h, "mesh registration", T0, T);
    if (rc) return rc;
    int shift = 0;
    rc = mesh_registration_setup(h, m, "mesh registration", P, F, shift);
    if (rc) return rc;
    const TriGrid &M = m->G;
    const double md2 = (double)P.max_dist * (double)P.max_dist;
    const size_t N = h->n;
    const int nq = h->hmeta.n_sorted;
    auto &G = h->registration;
    const size_t evals = (size_t)iterations + 1;
    rc = chain_open(h, evals, T);
    if (rc) return rc;
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.ctl.p);
    /* grid-stride under MESH_REG_GRID_CUS workgroups per compute unit (0: a thread per query); the words do not depend on it */
    const size_t cap = MESH_REG_GRID_CUS ? (size_t)MESH_REG_GRID_CUS * (size_t)h->num_cus : (size_t)0x7fffffff;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)std::max(nq, 0) + ICP_T - 1) / ICP_T, cap));
#if MESH_REG_SPLIT
    HIPCHK(h, G.key.ensure(std::max<size_t>((size_t)std::max(nq, 0), 1))); /* the winning record per query (the trimmed chain's key buffer) */
    const unsigned gsearch = (unsigned)std::max<size_t>(1, ((size_t)std::max(nq, 0) + TM_T - 1) / TM_T);
#endif
    for (int k = 0; k <= iterations; ++k) {
#if MESH_REG_SPLIT
        LAUNCH(h, "k_mesh_reg_search", k_mesh_reg_search, gsearch, TM_T, 0, (const float4 *)h->sorted4.p, nq, M, md2, G.T.p + 12 * (size_t)k, ctl, G.key.p);
        LAUNCH(h, "k_mesh_reg_sum", k_mesh_reg_sum, grid, ICP_T, 0, (const float4 *)h->sorted4.p, nq, M, F, G.T.p + 12 * (size_t)k, ctl, G.key.p,
               G.acc.p + ICP_WORDS * (size_t)k);
#else
        LAUNCH(h, "k_mesh_reg_terms", k_mesh_reg_terms, grid, ICP_T, 0, (const float4 *)h->sorted4.p, nq, M, F, md2, G.T.p + 12 * (size_t)k, ctl,
               G.acc.p + ICP_WORDS * (size_t)k);
#endif
        if (k < iterations)
            LAUNCH(h, "k_reg_step", k_reg_step, 1, 64, 0, G.acc.p + ICP_WORDS * (size_t)k, F, G.T.p + 12 * (size_t)k, G.rows.p + k, ctl);
    }
    IcpCtl C;
    std::vector<ppp_registration_row> R;
    rc = chain_collect(h, "mesh registration", iterations, nq, C, R);
    if (rc) return rc;
    if (stats) *stats = registration_stats(R, C, N, (size_t)nq, shift, F.c, F.Ln);
    const size_t k = std::min(row_cap, (size_t)C.steps + 1);
    if (rows && k) memcpy(rows, R.data(), k * sizeof(ppp_registration_row));
    return PPP_OK;
}

int ppp_get_mesh_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T12, ppp_registration_row *row,
                                    ppp_registration_stats *stats)
{
    return mesh_registration_chain(h, m, rp, T12, false, row, row ? 1 : 0, stats);
}

int ppp_register_mesh(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T0_12, ppp_registration_row *rows, size_t row_cap,
                      ppp_registration_stats *stats)
{
    return mesh_registration_chain(h, m, rp, T0_12, true, rows, row_cap, stats);
}

/* ---- the mesh calls for the points a handle owns (ppp_mesh_tile.h) ---- */

/* The exact deviation map of the points h owns (B.144-B.146): the plan, the range check on the host, the index, then k_mesht_fill,
   k_mesht_nearest, k_mesht_sign in the signed call, k_mesht_stats, k_devt_smooth where asked and k_devt_target back to back on the
   scan's stream, and one wait.  The mesh is whole: nothing on its side is checked against a range.  The buffers are
   ppp_get_mesh_deviation's: nothing is kept. */
struct MeshTileSignMaps { unsigned char *feature, *flags; ppp_mesh_signed_deviation_tile_stats *part; };
static int mesh_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp, const MeshTileSignMaps *sign, double *deviation, double *smoothed,
                               double *distance, int *tri_index, unsigned char *region, unsigned char *status, double *target, unsigned char *owned,
                               size_t cap, ppp_mesh_deviation_tile_stats *part)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const std::string w = sign ? "mesh signed deviation tile" : "mesh deviation tile";
    if (!m || !dp) return fail(h, PPP_ERR_ARG, w + ": no mesh or no parameters");
    int rc = deviation_params_ok(h, *dp, w, nullptr);
    if (rc) return rc;
    if (m->device != h->device) return fail(h, PPP_ERR_ARG, w + ": the mesh is on another device than the handle");
    const ppp_deviation_params P = *dp;
    const bool smooth = P.smooth_radius > 0.f;
    rc = deviation_side_cloud(h, h, w + ": the scan", true);
    if (rc) return rc;
    const size_t N = h->n;
    if (deviation_sum_overflows(P, N)) return fail(h, PPP_ERR_ARG, w + ": max_dist 2^24 n reaches 2^62: the smoothing's integer sum could overflow");
    /* from the plan alone, before an index is built or a kernel launched: what is evaluated is the owned interval widened by
       smooth_radius, and the scan's handle must index it */
    TileRange T;
    rc = tile_range(h, 0.f, T);
    if (rc) return rc;
    widened(T, P.smooth_radius, T.ev_lo, T.ev_hi);
    if (leaves_indexed_range(h, T.ev_lo, T.ev_hi))
        return fail(h, PPP_ERR_ARG, w + ": the owned interval widened by smooth_radius reaches beyond the scan's indexed slice range: raise range_margin");
    rc = deviation_side_index(h, h, w + ": the scan", false);
    if (rc) return rc;
    if (sign) { /* the topology on the mesh's stream, waited for: read-only from here on */
        rc = trimesh_topology_build(m, h);
        if (rc) return fail(h, rc, w + ": the mesh's topology could not be built");
        HIPCHK(h, hipSetDevice(h->device));
    }
    int pos0, pos1, hb0, hb1;
    rc = tile_positions(h, T, pos0, pos1);
    if (rc) return rc;
    sorted_slabs(h, hb0, hb1);
    auto &D = h->deviation;
    const size_t N1 = std::max<size_t>(N, 1);
    HIPCHK(h, D.dev.ensure(N1)); HIPCHK(h, D.target.ensure(N1)); HIPCHK(h, D.fix.ensure(N1)); HIPCHK(h, D.d2.ensure(N1)); HIPCHK(h, D.dist.ensure(N1));
    HIPCHK(h, D.ref_index.ensure(N1)); HIPCHK(h, D.status.ensure(N1)); HIPCHK(h, D.region.ensure(N1)); HIPCHK(h, D.owned.ensure(N1));
    HIPCHK(h, D.acc.ensure(DEV_ACC_WORDS)); HIPCHK(h, D.macc.ensure(MESHT_ACC_WORDS));
    if (smooth) HIPCHK(h, D.smoothed.ensure(N1));
    if (sign) { HIPCHK(h, D.feature.ensure(N1)); HIPCHK(h, D.flags.ensure(N1)); }
    double *v = smooth ? D.smoothed.p : D.dev.p;
    HIPCHK(h, hipMemsetAsync(D.acc.p, 0, DEVT_ACC_WORDS * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(D.macc.p, 0, MESHT_ACC_WORDS * sizeof(unsigned long long), h->stream));
    const size_t cap_grid = 2 * (size_t)h->num_cus;
    LAUNCH(h, "k_mesht_fill", k_mesht_fill, (unsigned)std::min<size_t>((N1 + TM_T - 1) / TM_T, cap_grid), TM_T, 0, (int)N, D.dev.p,
           smooth ? D.smoothed.p : nullptr, D.target.p, D.dist.p, D.ref_index.p, D.region.p, sign ? D.feature.p : nullptr, sign ? D.flags.p : nullptr,
           D.status.p, D.owned.p);
    if (pos1 > pos0) {
        const size_t gq = ((size_t)(pos1 - pos0) + TM_T - 1) / TM_T;
        static_assert(TM_T == DEV_T, "one grid for the search and the smoothing");
        const TmOut O = trimesh_outputs(D.dist.p, nullptr, D.dev.p, D.fix.p, D.d2.p, D.ref_index.p, D.region.p, D.status.p);
        LAUNCH(h, "k_mesht_nearest", k_mesht_nearest, (unsigned)gq, TM_T, 0, (const float4 *)h->sorted4.p, pos0, pos1, T, m->G,
               (double)P.max_dist * (double)P.max_dist, O, D.owned.p);
        if (sign) { /* the signed distance takes the deviation's place, in the map and in its fixed-point term, before the smoothing reads them */
            TmSignOut SO;
            SO.signed_distance = D.dev.p; SO.pseudonormal = nullptr; SO.dev = nullptr; SO.fix = D.fix.p; SO.feature = D.feature.p; SO.flags = D.flags.p;
            SO.tri_index = D.ref_index.p; SO.status = D.status.p;
            LAUNCH(h, "k_mesht_sign", k_mesht_sign, (unsigned)gq, TM_T, 0, (const float4 *)h->sorted4.p, pos0, pos1, T, m->G, m->T, SO);
        }
        LAUNCH(h, "k_mesht_stats", k_mesht_stats, (unsigned)std::min(gq, cap_grid), TM_T, 0, (const float4 *)h->sorted4.p, pos0, pos1, T, D.status.p,
               D.region.p, D.dist.p, sign ? D.flags.p : nullptr, D.dev.p, D.macc.p);
        if (smooth)
            LAUNCH(h, "k_devt_smooth", k_devt_smooth, (unsigned)gq, DEV_T, 0, contact_index(h), pos0, pos1, T, hb0, hb1,
                   P.smooth_radius * P.smooth_radius, D.status.p, D.fix.p, D.smoothed.p);
        LAUNCH(h, "k_devt_target", k_devt_target, (unsigned)std::min(gq, cap_grid), DEV_T, 0, h->sorted4.p, pos0, pos1, T, D.status.p, D.dev.p, v,
               D.d2.p, D.ref_index.p, P.allowance, P.gain, D.target.p, D.acc.p);
    }
    unsigned long long acc[DEVT_ACC_WORDS], macc[MESHT_ACC_WORDS];
    HIPCHK(h, copy_sync(h, acc, D.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
    HIPCHK(h, copy_sync(h, macc, D.macc.p, sizeof(macc), hipMemcpyDeviceToHost));
    const unsigned long long own = acc[0] + acc[1] + acc[2];
    if (own + acc[DEVT_ACC_HALO] > (unsigned long long)(pos1 - pos0) || acc[DEV_ACC_PROUD] > acc[0] || acc[DEV_ACC_BELOW] > acc[0] ||
        macc[0] + macc[1] + macc[2] != acc[0] || macc[MESHT_ACC_SIGN + 3] + macc[MESHT_ACC_SIGN + 4] > acc[0])
        return fail(h, PPP_ERR_HIP, w + ": statistics corrupt");
    ppp_mesh_deviation_tile_stats st = {};
    dev_stats_words(st.dev, N, acc);
    st.dev.owned = (size_t)own; st.dev.evaluated = (size_t)(own + acc[DEVT_ACC_HALO]);
    if (st.dev.matched) st.dev.fix_sum = (long long)acc[DEV_ACC_FIXSUM];
    st.dev.own_lo = T.own_lo; st.dev.own_hi = T.own_hi;
    st.dev.sum_parts = MapParts(h, N).grid;
    st.on_face = (size_t)macc[0]; st.on_edge = (size_t)macc[1]; st.on_vertex = (size_t)macc[2];
    st.max_distance = (double)NAN;
    if (st.dev.matched) memcpy(&st.max_distance, &macc[MESHT_ACC_FAR], sizeof(double));
    if (part) *part = st;
    if (sign && sign->part) {
        ppp_mesh_signed_deviation_tile_stats &ss = *sign->part;
        ss = ppp_mesh_signed_deviation_tile_stats{};
        ss.mesh = st;
        ss.on_border = (size_t)macc[MESHT_ACC_SIGN]; ss.irregular = (size_t)macc[MESHT_ACC_SIGN + 1]; ss.fallback = (size_t)macc[MESHT_ACC_SIGN + 2];
        ss.negative = (size_t)macc[MESHT_ACC_SIGN + 3]; ss.positive = (size_t)macc[MESHT_ACC_SIGN + 4];
    }
    const size_t k = std::min(cap, N);
    rc = deviation_copy_out(h, k, v, deviation, smoothed, tri_index, status, target, owned);
    if (rc) return rc;
    if (distance && k) HIPCHK(h, copy_sync(h, distance, D.dist.p, k * sizeof(double), hipMemcpyDeviceToHost));
    if (region && k) HIPCHK(h, copy_sync(h, region, D.region.p, k, hipMemcpyDeviceToHost));
    if (sign && sign->feature && k) HIPCHK(h, copy_sync(h, sign->feature, D.feature.p, k, hipMemcpyDeviceToHost));
    if (sign && sign->flags && k) HIPCHK(h, copy_sync(h, sign->flags, D.flags.p, k, hipMemcpyDeviceToHost));
    return PPP_OK;
}

int ppp_get_mesh_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp, double *deviation, double *smoothed, double *distance,
                                int *tri_index, unsigned char *region, unsigned char *status, double *target, unsigned char *owned, size_t cap,
                                ppp_mesh_deviation_tile_stats *part)
{
    return mesh_deviation_tile(h, m, dp, nullptr, deviation, smoothed, distance, tri_index, region, status, target, owned, cap, part);
}

int ppp_get_mesh_signed_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp, double *signed_distance, double *smoothed,
                                       double *distance, int *tri_index, unsigned char *region, unsigned char *feature, unsigned char *flags,
                                       unsigned char *status, double *target, unsigned char *owned, size_t cap,
                                       ppp_mesh_signed_deviation_tile_stats *part)
{
    const MeshTileSignMaps sign = {feature, flags, part};
    return mesh_deviation_tile(h, m, dp, &sign, signed_distance, smoothed, distance, tri_index, region, status, target, owned, cap, nullptr);
}

/* The merges (B.147; host only): dev by ppp_merge_deviation_tiles' own routine, which also refuses what it refuses; the counts
   add; max_distance is the maximum of the parts that matched (doubles >= +0 order as their bits), the NaN when none did.  A part
   whose counts by region do not add up to its matched points is not a tile's. */
int ppp_merge_mesh_deviation_tiles(size_t tiles, const ppp_mesh_deviation_tile_stats *parts, const double *const *v, const unsigned char *const *status,
                                   const double *const *target, const unsigned char *const *owned, ppp_mesh_deviation_stats *stats)
{
    if (!tiles || !parts || !stats) return PPP_ERR_ARG;
    std::vector<ppp_deviation_tile_stats> dev(tiles);
    ppp_mesh_deviation_stats st = {};
    unsigned long long far = 0;
    for (size_t t = 0; t < tiles; ++t) {
        const ppp_mesh_deviation_tile_stats &p = parts[t];
        dev[t] = p.dev;
        if (p.on_face + p.on_edge + p.on_vertex != p.dev.matched) return PPP_ERR_ARG;
        st.on_face += p.on_face; st.on_edge += p.on_edge; st.on_vertex += p.on_vertex;
        if (!p.dev.matched) continue;
        if (!(p.max_distance >= 0.0)) return PPP_ERR_ARG; /* (a NaN too) */
        unsigned long long bits;
        memcpy(&bits, &p.max_distance, sizeof(bits));
        far = std::max(far, bits & 0x7fffffffffffffffull); /* (-0 as +0) */
    }
    const int rc = ppp_merge_deviation_tiles(tiles, dev.data(), v, status, target, owned, &st.dev);
    if (rc) return rc;
    st.max_distance = (double)NAN;
    if (st.dev.matched) memcpy(&st.max_distance, &far, sizeof(double));
    *stats = st;
    return PPP_OK;
}

int ppp_merge_mesh_signed_deviation_tiles(size_t tiles, const ppp_mesh_signed_deviation_tile_stats *parts, const double *const *v,
                                          const unsigned char *const *status, const double *const *target, const unsigned char *const *owned,
                                          ppp_mesh_signed_deviation_stats *stats)
{
    if (!tiles || !parts || !stats) return PPP_ERR_ARG;
    std::vector<ppp_mesh_deviation_tile_stats> mesh(tiles);
    ppp_mesh_signed_deviation_stats st = {};
    for (size_t t = 0; t < tiles; ++t) {
        const ppp_mesh_signed_deviation_tile_stats &p = parts[t];
        mesh[t] = p.mesh;
        if (p.negative + p.positive > p.mesh.dev.matched || p.on_border > p.mesh.dev.matched || p.irregular > p.mesh.dev.matched ||
            p.fallback > p.mesh.dev.matched)
            return PPP_ERR_ARG;
        st.on_border += p.on_border; st.irregular += p.irregular; st.fallback += p.fallback; st.negative += p.negative; st.positive += p.positive;
    }
    const int rc = ppp_merge_mesh_deviation_tiles(tiles, mesh.data(), v, status, target, owned, &st.mesh);
    if (rc) return rc;
    *stats = st;
    return PPP_OK;
}

/* What a tile of a mesh registration needs before its first evaluation (B.148): the checks, the plan, the scan's index, the frame
   from the mesh's box (B.126) and the shift of the WHOLE scan (B.68), the positions, the grids, the buffers, and the frame on the
   device.  The mesh is whole and read-only since its create call waited: no range condition, nothing to build on its side. */
static int mesht_prepare(RegtTile &t, const ppp_registration_params &P, IcpFrame F)
{
    ppp_handle h = t.h;
    HIPCHK(h, hipSetDevice(h->device));
    if (t.mesh->device != h->device) return fail(h, PPP_ERR_ARG, "mesh registration tile: the mesh is on another device than the handle");
    int rc = deviation_side_cloud(h, h, "mesh registration tile: the scan", true);
    if (rc) return rc;
    const int shift = icp_shift(h->n, F.md2);
    if (shift < 16) return fail(h, PPP_ERR_ARG, "mesh registration tile: fewer than 16 fractional bits are left (n max_dist^2 too large): the integer sums could overflow");
    rc = tile_range(h, 0.f, t.own);
    if (rc) return rc;
    rc = deviation_side_index(h, h, "mesh registration tile: the scan", false);
    if (rc) return rc;
    float mn[3], mx[3];
    mesh_box_floats(t.mesh->G, mn, mx);
    frame_from_bounds(mn, mx, (double)P.max_dist, shift, F.c, &F.Ln, &F.scale);
    rc = tile_positions(h, t.own, t.pos0, t.pos1);
    if (rc) return rc;
    const size_t np = (size_t)(t.pos1 - t.pos0);
    const size_t cap = MESH_REG_GRID_CUS ? (size_t)MESH_REG_GRID_CUS * (size_t)h->num_cus : (size_t)0x7fffffff;
    t.grid = (unsigned)std::max<size_t>(1, std::min<size_t>((np + ICP_T - 1) / ICP_T, cap));
    t.gsearch = (unsigned)std::max<size_t>(1, (np + TM_T - 1) / TM_T);
    ppp_registration_part &p = t.part;
    p = ppp_registration_part{};
    p.evaluated = np;
    p.own_lo = t.own.own_lo; p.own_hi = t.own.own_hi;
    p.n = h->n; p.shift = shift;
    for (int d = 0; d < 3; ++d) p.centre[d] = F.c[d];
    p.length = F.Ln;
    auto &G = h->registration;
    HIPCHK(h, G.T.ensure(12)); HIPCHK(h, G.acc.ensure(REGT_WORDS)); HIPCHK(h, G.tframe.ensure(1)); HIPCHK(h, G.tpin.ensure(REGT_WORDS + 12));
    HIPCHK(h, G.key.ensure(std::max<size_t>(np, 1))); /* the winning record per position (the whole-cloud chain's buffer) */
    HIPCHK(h, copy_sync(h, G.tframe.p, &F, sizeof(F), hipMemcpyHostToDevice));
    return PPP_OK;
}

/* one evaluation of a tile at T, enqueued on its handle's stream: T to the device, the words cleared, k_mesht_reg_search,
   k_mesht_reg_sum, the words back to pinned memory.  Nobody waits here. */
static int mesht_enqueue(RegtTile &t, const double *T, double md2)
{
    ppp_handle h = t.h;
    auto &G = h->registration;
    HIPCHK(h, hipSetDevice(h->device));
    memcpy(regt_pinned_T(t), T, 12 * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(G.T.p, regt_pinned_T(t), 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, REGT_WORDS * sizeof(unsigned long long), h->stream));
    if (t.pos1 > t.pos0) {
        LAUNCH(h, "k_mesht_reg_search", k_mesht_reg_search, t.gsearch, TM_T, 0, (const float4 *)h->sorted4.p, t.pos0, t.pos1, t.own, t.mesh->G, md2, G.T.p,
               G.key.p);
        LAUNCH(h, "k_mesht_reg_sum", k_mesht_reg_sum, t.grid, ICP_T, 0, (const float4 *)h->sorted4.p, t.pos0, t.pos1, t.own, t.mesh->G, G.tframe.p, G.T.p,
               G.key.p, G.acc.p);
    }
    HIPCHK(h, hipMemcpyAsync(G.tpin.p, G.acc.p, REGT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    return PPP_OK;
}

/* the wait for a tile's evaluation, and its row: the words' sanity, the terms.  No refusal: the mesh is whole. */
static int mesht_collect(RegtTile &t, const double *T, ppp_registration_row *row)
{
    ppp_handle h = t.h;
    int rc = regt_wait(t);
    if (rc) return rc;
    const unsigned long long *w = h->registration.tpin.p;
    if (w[REGT_OWNED] > (unsigned long long)(t.pos1 - t.pos0) || w[ICP_PAIRS] > w[REGT_OWNED]) return fail(h, PPP_ERR_HIP, "mesh registration tile: sums corrupt");
    t.part.owned = (size_t)w[REGT_OWNED];
    *row = ppp_registration_row{};
    icp_row_terms(row, T, w);
    return PPP_OK;
}

int ppp_get_mesh_registration_terms_tile(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T12, ppp_registration_row *row,
                                         ppp_registration_part *part)
{
    IcpFrame F = {};
    double T[12];
    int rc = regt_call_ok(h, rp, T12, F, T);
    if (rc) return rc;
    if (!m) return fail(h, PPP_ERR_ARG, "mesh registration tile: no mesh");
    RegtTile t;
    t.h = h; t.mesh = m;
    rc = mesht_prepare(t, *rp, F);
    if (rc) return rc;
    rc = mesht_enqueue(t, T, (double)rp->max_dist * (double)rp->max_dist);
    if (rc) return rc;
    ppp_registration_row r;
    rc = mesht_collect(t, T, &r);
    if (rc) return rc;
    if (row) *row = r;
    if (part) *part = t.part;
    return PPP_OK;
}

/* do two meshes hold one surface as the frame and the search see it?  the triangle counts and the box, bit for bit */
static bool mesht_same_mesh(const ppp_trimesh a, const ppp_trimesh b)
{
    return a->n_tris == b->n_tris && a->G.indexed == b->G.indexed && memcmp(a->G.mn, b->G.mn, sizeof(a->G.mn)) == 0 && memcmp(a->G.mx, b->G.mx, sizeof(a->G.mx)) == 0;
}

/* The tiled loop against the mesh (B.149): ppp_register_tiles's, with the mesh in every reference's place -- regt_loop with an
   evaluation that is k_mesht_reg_search and k_mesht_reg_sum per tile, one copy back and one wait per tile, then the merge and the
   step on the host. */
int ppp_register_mesh_tiles(const ppp_handle *hs, const ppp_trimesh *ms, size_t count, const ppp_registration_params *rp, const double *T0_12,
                            ppp_registration_row *rows, size_t row_cap, ppp_register_tiles_stats *stats)
{
    if (stats) { *stats = ppp_register_tiles_stats{}; stats->failed_tile = -1; }
    if (!hs || !ms || !count || !hs[0]) return PPP_ERR_ARG;
    ppp_handle h0 = hs[0];
    IcpFrame F = {};
    double T[12];
    int rc = regt_call_ok(h0, rp, T0_12, F, T);
    if (rc) return rc;
    const ppp_registration_params P = *rp;
    const double md2 = (double)P.max_dist * (double)P.max_dist;
    RegtCall call = {"mesh registration tiles", stats};
    if (!rows && row_cap) return fail(h0, PPP_ERR_ARG, "mesh registration tiles: rows is NULL with row_cap > 0");
    for (size_t i = 0; i < count; ++i) {
        if (!hs[i] || !ms[i]) return fail(h0, PPP_ERR_ARG, "mesh registration tiles: a NULL handle or mesh");
        for (size_t k = 0; k < i; ++k) if (hs[k] == hs[i]) return fail(h0, PPP_ERR_ARG, "mesh registration tiles: a scan handle stands in two slots");
        if (!mesht_same_mesh(ms[i], ms[0])) return fail(h0, PPP_ERR_ARG, "mesh registration tiles: the meshes disagree on their triangles or their box");
    }
    call.tiles.assign(count, RegtTile()); call.part_rows.resize(count); call.parts.resize(count);
    for (size_t i = 0; i < count; ++i) {
        RegtTile &t = call.tiles[i];
        t.h = hs[i]; t.mesh = ms[i];
        rc = mesht_prepare(t, P, F);
        if (rc) return call.failed(i, rc);
    }
    std::vector<ppp_registration_row> R;
    IcpCtl C = {};
    rc = regt_loop(P, F, T, R, C, call.whole, [&](int, ppp_registration_row &rw) {
        const int e = regt_pass(call, [&](RegtTile &t) { return mesht_enqueue(t, T, md2); }, [&](RegtTile &t, size_t i) {
            const int ec = mesht_collect(t, T, &call.part_rows[i]);
            call.parts[i] = t.part;
            return ec;
        });
        return e ? e : regt_merged(h0, call, T, rw);
    });
    if (rc) return rc;
    if (stats) stats->reg = registration_stats(R, C, call.whole.n, call.whole.owned, call.whole.shift, call.whole.centre, call.whole.length);
    const size_t k = std::min(row_cap, (size_t)C.steps + 1);
    if (rows && k) memcpy(rows, R.data(), k * sizeof(ppp_registration_row));
    return PPP_OK;
}

/* The area moments of the mesh.  mesh_moments_frame: the centre, the length and the fixed point of B.135
   from the mesh's box; mesh_moments_result: the frame the ten words imply.  ppp_trimesh_get_moments runs k_mesh_moments on the
   mesh's own stream into the mesh's own ten words, under a lock (calls on one mesh from several threads take turns), and waits
   once; no handle: an error is its code.  ppp_register_mesh_global runs the same kernel on h's stream into h's words, under h's
   kernel timers (handle_mesh_moments): the mesh is read-only, so either stream gives the same words. */
static bool mesh_moments_frame(ppp_trimesh m, MomFrame &F, int &ms)
{
    ms = mesh_mom_shift((size_t)m->n_tris);
    float mn[3], mx[3];
    mesh_box_floats(m->G, mn, mx);
    frame_from_bounds(mn, mx, 0.0, ms, F.c, &F.L, &F.scale); /* (+ 0.0 changes no bit of an extent) */
    return F.L > 0.0 && std::isfinite(F.L);
}

static unsigned mesh_moments_grid(ppp_trimesh m, int num_cus)
{
    return (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)m->G.indexed + MOM_T - 1) / MOM_T, 2 * (size_t)num_cus));
}

static bool mesh_moments_result(ppp_trimesh m, const unsigned long long *acc, const MomFrame &F, int ms, ppp_cloud_frame *frame)
{
    long long words[MOM_WORDS];
    for (int i = 0; i < MOM_WORDS; ++i) words[i] = (long long)acc[i];
    return mesh_frame_from_words(words, (size_t)m->G.indexed, ms, F.c, F.L, frame);
}

int ppp_trimesh_get_moments(ppp_trimesh m, ppp_cloud_frame *frame)
{
    if (!m || !frame) return PPP_ERR_ARG;
    MomFrame F;
    int ms = 0;
    if (!mesh_moments_frame(m, F, ms)) return PPP_ERR_ARG;
    unsigned long long acc[MOM_WORDS];
    {
        std::lock_guard<std::mutex> lock(m->mom_lock);
        if (hipSetDevice(m->device) != hipSuccess || m->mom.ensure(MOM_WORDS) != hipSuccess) return PPP_ERR_HIP;
        if (hipMemsetAsync(m->mom.p, 0, sizeof(acc), m->stream) != hipSuccess) return PPP_ERR_HIP;
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_mesh_moments, dim3(mesh_moments_grid(m, m->num_cus)), dim3(MOM_T), 0, m->stream, m->G, F, m->mom.p);
        if (hipGetLastError() != hipSuccess) return PPP_ERR_HIP;
        if (hipMemcpyAsync(acc, m->mom.p, sizeof(acc), hipMemcpyDeviceToHost, m->stream) != hipSuccess) return PPP_ERR_HIP;
        if (hipStreamSynchronize(m->stream) != hipSuccess) return PPP_ERR_HIP;
    }
    return mesh_moments_result(m, acc, F, ms, frame) ? PPP_OK : PPP_ERR_ARG;
}

/* the mesh's area frame for a call on h (w: its name): k_mesh_moments on h's stream into h's ten words, one wait */
static int handle_mesh_moments(ppp_handle h, ppp_trimesh m, const std::string &w, ppp_cloud_frame *frame)
{
    MomFrame F;
    int ms = 0;
    if (!mesh_moments_frame(m, F, ms)) return fail(h, PPP_ERR_ARG, w + ": the box of the mesh has no extent (L == 0)");
    auto &G = h->registration;
    HIPCHK(h, G.mom.ensure(MOM_WORDS));
    HIPCHK(h, hipMemsetAsync(G.mom.p, 0, MOM_WORDS * sizeof(unsigned long long), h->stream));
    LAUNCH(h, "k_mesh_moments", k_mesh_moments, mesh_moments_grid(m, h->num_cus), MOM_T, 0, m->G, F, G.mom.p);
    unsigned long long acc[MOM_WORDS];
    HIPCHK(h, copy_sync(h, acc, G.mom.p, sizeof(acc), hipMemcpyDeviceToHost));
    if (!mesh_moments_result(m, acc, F, ms, frame))
        return fail(h, PPP_ERR_ARG, w + ": the mesh has no area at its moments' fixed point (W0 <= 0)");
    return PPP_OK;
}

int ppp_mesh_frame_from_moments(const long long *words10, int ms, const double *c3, double L, ppp_cloud_frame *frame)
{
    if (!words10 || !c3 || !frame) return PPP_ERR_ARG;
    return mesh_frame_from_words(words10, 0, ms, c3, L, frame) ? PPP_OK : PPP_ERR_ARG; /* (the words do not hold the count) */
}

/* Global registration to the mesh: ppp_register_global's shape with the mesh in the reference's place -- the
   scan's point moments and the mesh's area moments, the starts the two frames imply, then every start's coarse chain side by
   side: coarse.iterations + 1 launches each of k_mesh_reg_search_multi and k_mesh_reg_sum_multi and coarse.iterations of
   k_reg_step_multi back to back on h's stream, on the queries compacted once -- one wait, the winner by cost on the host, and
   mesh_registration_chain from it. */
int ppp_register_mesh_global(ppp_handle h, ppp_trimesh m, const ppp_global_registration_params *gp, ppp_registration_candidate *cands, size_t cand_cap,
                             ppp_registration_row *rows, size_t row_cap, ppp_global_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const char *w = "mesh global registration";
    if (!m || !gp) return fail(h, PPP_ERR_ARG, std::string(w) + ": no mesh or no parameters");
    const ppp_global_registration_params P = *gp;
    IcpFrame F, Ffine;
    int rc = global_params_ok(h, w, P, cands, cand_cap, rows, row_cap, F, Ffine);
    if (rc) return rc;
    int shift = 0;
    rc = mesh_registration_setup(h, m, w, P.coarse, F, shift);
    if (rc) return rc;
    if (icp_shift(h->n, Ffine.md2) < 16)
        return fail(h, PPP_ERR_ARG, std::string(w) + ": fewer than 16 fractional bits are left (n max_dist^2 too large): the integer sums could overflow");
    ppp_global_registration_stats st = {};
    rc = cloud_moments(h, h, "the scan", &st.scan);
    if (rc) return rc;
    rc = handle_mesh_moments(h, m, w, &st.ref);
    if (rc) return rc;
    CoarseStage S;
    rc = coarse_open(h, w, P, st.scan, st.ref, S);
    if (rc) return rc;
    const int K = S.K, nq = S.nq;
    auto &G = h->registration;
    const TriGrid &M = m->G;
    const double md2 = (double)P.coarse.max_dist * (double)P.coarse.max_dist;
    HIPCHK(h, G.mwin.ensure((size_t)K * (size_t)nq)); /* the winning record per start and query */
    const unsigned gsearch = (unsigned)(((size_t)nq + TM_T - 1) / TM_T);
    /* the sum: all starts together under MESH_REG_GRID_CUS workgroups per CU (0: no cap), and never below one per start */
    const size_t cap = MESH_REG_GRID_CUS ? (size_t)MESH_REG_GRID_CUS * (size_t)h->num_cus / (size_t)K : (size_t)0x7fffffff;
    const size_t per = std::max<size_t>(1, std::min<size_t>(((size_t)nq + ICP_T - 1) / ICP_T, cap));
    for (int k = 0; k <= S.iterations; ++k) {
        LAUNCH(h, "k_mesh_reg_search_multi", k_mesh_reg_search_multi, dim3(gsearch, (unsigned)K), TM_T, 0, (const float4 *)G.queries.p, nq, M, md2,
               G.mT.p + 12 * (size_t)k, S.tstride, S.ctl, G.mwin.p);
        LAUNCH(h, "k_mesh_reg_sum_multi", k_mesh_reg_sum_multi, dim3((unsigned)per, (unsigned)K), ICP_T, 0, (const float4 *)G.queries.p, nq, M, F,
               G.mT.p + 12 * (size_t)k, S.tstride, S.ctl, G.mwin.p, G.macc.p + ICP_WORDS * (size_t)k, S.astride);
        if (k < S.iterations)
            LAUNCH(h, "k_reg_step_multi", k_reg_step_multi, K, 64, 0, G.macc.p + ICP_WORDS * (size_t)k, S.astride, F, G.mT.p + 12 * (size_t)k, S.tstride,
                   G.mrows.p + k, S.evals, S.ctl);
    }
    rc = coarse_collect(h, w, F, S);
    if (rc) return rc;
    rc = mesh_registration_chain(h, m, &P.fine, S.cands[(size_t)S.winner].T, true, rows, row_cap, &st.fine);
    if (rc) return rc;
    global_results(S, shift, st, stats, cands, cand_cap);
    return PPP_OK;
}

/* The robust mesh chain: mesh_registration_chain's setup -- the scan's slab index, the frame from the mesh's box,
   ppp_register's shift -- and robust_chain's shape on it: robust_open, then iterations + 1 evaluations (k_mesh_rob_pair, the walk
   paid once; k_mesh_rob_digit0, unless the walk counts the digit itself: MESH_ROB_DIGIT_PASS; k_trim_narrow<1> and <2> at keep 0.5; k_mesh_rob_terms) and
   iterations steps (k_reg_step on the 30 words: `used` is word 0) back to back on the scan's stream, k_rob_scatter, and
   robust_collect's one wait.  !loop: the one evaluation of ppp_get_mesh_robust_registration_terms. */
static int mesh_robust_chain(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T0, bool loop,
                             ppp_robust_registration_row *rows, size_t row_cap, unsigned char *status, float *weight, double *residual, size_t cap,
                             ppp_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!m || !bp) return fail(h, PPP_ERR_ARG, "robust mesh registration: no mesh or no parameters");
    if (!rows && row_cap) return fail(h, PPP_ERR_ARG, "robust mesh registration: rows is NULL with row_cap > 0");
    int rc = robust_params_ok(h, "robust mesh registration", bp);
    if (rc) return rc;
    const ppp_registration_params P = bp->icp;
    const RobScale S = {bp->tune, bp->sigma_min};
    IcpFrame F;
    rc = registration_params_ok(h, P, F);
    if (rc) return rc;
    const int iterations = loop ? P.iterations : 0;
    double T[12];
    rc = opening_transform(h, "robust mesh registration", T0, T);
    if (rc) return rc;
    int shift = 0;
    rc = mesh_registration_setup(h, m, "robust mesh registration", P, F, shift);
    if (rc) return rc;
    const TriGrid &M = m->G;
    const double md2 = (double)P.max_dist * (double)P.max_dist;
    const int nq = h->hmeta.n_sorted;
    const size_t nqs = (size_t)std::max(nq, 0);
    auto &G = h->registration;
    const size_t evals = (size_t)iterations + 1;
    HIPCHK(h, G.mwin.ensure(std::max<size_t>(nqs, 1)));
    rc = robust_open(h, evals, nq, T);
    if (rc) return rc;
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.ctl.p);
    TrimCut *cuts = reinterpret_cast<TrimCut *>(G.cuts.p);
    const unsigned gpair = (unsigned)std::max<size_t>(1, (nqs + TM_T - 1) / TM_T); /* a thread per query */
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((nqs + TRIM_T - 1) / TRIM_T, 2 * (size_t)h->num_cus));
    /* grid-stride under MESH_ROB_GRID_CUS workgroups per compute unit (0: a thread per query); the words do not depend on it */
    const size_t tcap = MESH_ROB_GRID_CUS ? (size_t)MESH_ROB_GRID_CUS * (size_t)h->num_cus : (size_t)0x7fffffff;
    const unsigned gterms = (unsigned)std::max<size_t>(1, std::min<size_t>((nqs + TRIM_T - 1) / TRIM_T, tcap));
    for (int k = 0; k <= iterations; ++k) {
        unsigned *hist = G.hist.p + TRIM_WORDS * (size_t)k;
        unsigned long long *acc = G.acc.p + ROB_WORDS * (size_t)k;
        LAUNCH(h, "k_mesh_rob_pair", k_mesh_rob_pair, gpair, TM_T, 0, (const float4 *)h->sorted4.p, nq, M, md2, G.T.p + 12 * (size_t)k, ctl, G.mwin.p,
               G.rres.p, G.key.p, hist);
#if MESH_ROB_DIGIT_PASS
        LAUNCH(h, "k_mesh_rob_digit0", k_mesh_rob_digit0, grid, TRIM_T, 0, G.key.p, nq, ctl, hist);
#endif
        LAUNCH(h, "k_trim_narrow<1>", k_trim_narrow<1>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist, hist + TRIM_B0, ROB_KEEP, cuts + k);
        LAUNCH(h, "k_trim_narrow<2>", k_trim_narrow<2>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist + TRIM_B0, hist + TRIM_B0 + TRIM_B1, ROB_KEEP, cuts + k);
        LAUNCH(h, "k_mesh_rob_terms", k_mesh_rob_terms, gterms, TRIM_T, 0, (const float4 *)h->sorted4.p, nq, M, F, S, G.T.p + 12 * (size_t)k, ctl, G.mwin.p,
               G.rres.p, G.key.p, hist + TRIM_B0 + TRIM_B1, cuts + k, G.rsigma.p + k, acc);
        if (k < iterations) LAUNCH(h, "k_reg_step", k_reg_step, 1, 64, 0, acc, F, G.T.p + 12 * (size_t)k, G.rows.p + k, ctl);
    }
    LAUNCH(h, "k_rob_scatter", k_rob_scatter, grid, TRIM_T, 0, h->sorted4.p, nq, G.key.p, G.rres.p, ctl, cuts, G.rsigma.p, S, (int)evals,
           (int)std::max<size_t>(h->n, 1), G.tstatus.p, G.td2.p, G.rresid.p);
    return robust_collect(h, "robust mesh registration", iterations, nq, shift, F, rows, row_cap, status, weight, residual, cap, stats);
}

int ppp_get_mesh_robust_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T12,
                                           ppp_robust_registration_row *row, unsigned char *status, float *weight, double *residual, size_t cap,
                                           ppp_registration_stats *stats)
{
    return mesh_robust_chain(h, m, bp, T12, false, row, row ? 1 : 0, status, weight, residual, cap, stats);
}

int ppp_register_mesh_robust(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T0_12,
                             ppp_robust_registration_row *rows, size_t row_cap, unsigned char *status, float *weight, double *residual, size_t cap,
                             ppp_registration_stats *stats)
{
    return mesh_robust_chain(h, m, bp, T0_12, true, rows, row_cap, status, weight, residual, cap, stats);
}

void ppp_default_mesh_trimmed_registration_params(ppp_mesh_trimmed_registration_params *mp)
{
    if (!mp) return;
    ppp_default_trimmed_registration_params(&mp->trim);
    mp->border = PPP_MESH_BORDER_PAIR;
}

/* The trimmed mesh chain: mesh_registration_chain's setup -- the scan's slab index, the frame from the mesh's box,
   ppp_register's shift -- and, under PPP_MESH_BORDER_REJECT, the mesh's welded topology where it is missing (on the mesh's stream,
   waited for: read-only from here on); then registration_chain's trimmed shape on it: iterations + 1 evaluations (k_mesh_trim_pair,
   the walk paid once; k_mesh_trim_digit0; k_trim_narrow<1> and <2> at keep; k_mesh_trim_terms) and iterations steps (k_reg_step on
   the kept pairs' 29 words) back to back on the scan's stream, k_mesh_trim_scatter, and chain_collect's one wait.  !loop: the one
   evaluation of ppp_get_mesh_trimmed_registration_terms. */
static int mesh_trimmed_chain(ppp_handle h, ppp_trimesh m, const ppp_mesh_trimmed_registration_params *mp, const double *T0, bool loop,
                              ppp_mesh_trimmed_registration_row *rows, size_t row_cap, unsigned char *status, float *d2, size_t cap,
                              ppp_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const char *w = "trimmed mesh registration";
    if (!m || !mp) return fail(h, PPP_ERR_ARG, std::string(w) + ": no mesh or no parameters");
    if (!rows && row_cap) return fail(h, PPP_ERR_ARG, std::string(w) + ": rows is NULL with row_cap > 0");
    const double keep = mp->trim.keep;
    if (!(keep > 0.0 && keep <= 1.0)) return fail(h, PPP_ERR_ARG, std::string(w) + ": keep must be in (0, 1]");
    if (mp->border != PPP_MESH_BORDER_PAIR && mp->border != PPP_MESH_BORDER_REJECT)
        return fail(h, PPP_ERR_ARG, std::string(w) + ": border must be PPP_MESH_BORDER_PAIR or PPP_MESH_BORDER_REJECT");
    const bool reject = mp->border == PPP_MESH_BORDER_REJECT;
    const ppp_registration_params P = mp->trim.icp;
    IcpFrame F;
    int rc = registration_params_ok(h, P, F);
    if (rc) return rc;
    const int iterations = loop ? P.iterations : 0;
    double T[12];
    rc = opening_transform(h, w, T0, T);
    if (rc) return rc;
    int shift = 0;
    rc = mesh_registration_setup(h, m, w, P, F, shift);
    if (rc) return rc;
    if (reject) {
        rc = trimesh_topology_build(m, h);
        if (rc) return fail(h, rc, std::string(w) + ": the mesh's topology could not be built");
        HIPCHK(h, hipSetDevice(h->device));
    }
    const TriGrid &M = m->G;
    const TriTopo topo = reject ? m->T : TriTopo{};
    const double md2 = (double)P.max_dist * (double)P.max_dist;
    const size_t N = h->n, N1 = std::max<size_t>(N, 1);
    const int nq = h->hmeta.n_sorted;
    const size_t nqs = (size_t)std::max(nq, 0);
    auto &G = h->registration;
    const size_t evals = (size_t)iterations + 1;
    rc = chain_open(h, evals, T);
    if (rc) return rc;
    static_assert(sizeof(TrimCut) == 8 * sizeof(unsigned), "TrimCut is eight words");
    HIPCHK(h, G.mwin.ensure(std::max<size_t>(nqs, 1))); HIPCHK(h, G.key.ensure(std::max<size_t>(nqs, 1)));
    HIPCHK(h, G.hist.ensure(TRIM_WORDS * evals)); HIPCHK(h, G.cuts.ensure(8 * evals));
    HIPCHK(h, G.tstatus.ensure(N1)); HIPCHK(h, G.td2.ensure(N1));
    /* every evaluation has histograms and a cut of its own: one clear on the stream before the chain, none between iterations */
    HIPCHK(h, hipMemsetAsync(G.hist.p, 0, TRIM_WORDS * evals * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(G.cuts.p, 0, 8 * evals * sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(G.tstatus.p, PPP_TRIM_DROPPED, N1, h->stream)); /* points outside the index: not finite */
    HIPCHK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(G.td2.p), (int)TRIM_NAN, N1, h->stream));
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.ctl.p);
    TrimCut *cuts = reinterpret_cast<TrimCut *>(G.cuts.p);
    const unsigned gpair = (unsigned)std::max<size_t>(1, (nqs + TM_T - 1) / TM_T); /* a thread per query */
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((nqs + TRIM_T - 1) / TRIM_T, 2 * (size_t)h->num_cus));
    /* grid-stride under MESH_TRIM_GRID_CUS workgroups per compute unit (0: a thread per query); the words do not depend on it */
    const size_t tcap = MESH_TRIM_GRID_CUS ? (size_t)MESH_TRIM_GRID_CUS * (size_t)h->num_cus : (size_t)0x7fffffff;
    const unsigned gterms = (unsigned)std::max<size_t>(1, std::min<size_t>((nqs + TRIM_T - 1) / TRIM_T, tcap));
    const float4 *q4 = (const float4 *)h->sorted4.p;
    for (int k = 0; k <= iterations; ++k) {
        unsigned *hist = G.hist.p + TRIM_WORDS * (size_t)k;
        const double *Tk = G.T.p + 12 * (size_t)k;
        if (reject) LAUNCH(h, "k_mesh_trim_pair<reject>", k_mesh_trim_pair<true>, gpair, TM_T, 0, q4, nq, M, topo, md2, Tk, ctl, G.mwin.p, G.key.p);
        else LAUNCH(h, "k_mesh_trim_pair<pair>", k_mesh_trim_pair<false>, gpair, TM_T, 0, q4, nq, M, topo, md2, Tk, ctl, G.mwin.p, G.key.p);
        LAUNCH(h, "k_mesh_trim_digit0", k_mesh_trim_digit0, grid, TRIM_T, 0, G.key.p, nq, ctl, hist, &cuts[k].pad);
        LAUNCH(h, "k_trim_narrow<1>", k_trim_narrow<1>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist, hist + TRIM_B0, keep, cuts + k);
        LAUNCH(h, "k_trim_narrow<2>", k_trim_narrow<2>, grid, TRIM_T, 0, G.key.p, nq, ctl, hist + TRIM_B0, hist + TRIM_B0 + TRIM_B1, keep, cuts + k);
        LAUNCH(h, "k_mesh_trim_terms", k_mesh_trim_terms, gterms, TRIM_T, 0, q4, nq, M, F, Tk, ctl, G.mwin.p, G.key.p, hist + TRIM_B0 + TRIM_B1, cuts + k,
               G.acc.p + ICP_WORDS * (size_t)k);
        if (k < iterations) LAUNCH(h, "k_reg_step", k_reg_step, 1, 64, 0, G.acc.p + ICP_WORDS * (size_t)k, F, G.T.p + 12 * (size_t)k, G.rows.p + k, ctl);
    }
    LAUNCH(h, "k_mesh_trim_scatter", k_mesh_trim_scatter, grid, TRIM_T, 0, q4, nq, G.key.p, ctl, cuts, (int)evals, (int)N1, G.tstatus.p, G.td2.p);
    IcpCtl C;
    std::vector<ppp_registration_row> R;
    rc = chain_collect(h, w, iterations, nq, C, R);
    if (rc) return rc;
    const size_t last = (size_t)C.steps;
    if (stats) *stats = registration_stats(R, C, N, (size_t)nq, shift, F.c, F.Ln);
    std::vector<TrimCut> cut(last + 1);
    HIPCHK(h, copy_sync(h, cut.data(), G.cuts.p, (last + 1) * sizeof(TrimCut), hipMemcpyDeviceToHost));
    for (size_t i = 0; i <= last; ++i)
        if ((size_t)cut[i].paired + (size_t)cut[i].pad > nqs || R[i].pairs > cut[i].paired || (cut[i].paired && R[i].pairs < cut[i].k) ||
            (!reject && cut[i].pad))
            return fail(h, PPP_ERR_HIP, std::string(w) + ": cut corrupt");
    const size_t k = std::min(row_cap, last + 1);
    for (size_t i = 0; rows && i < k; ++i) {
        memset(&rows[i], 0, sizeof(rows[i])); /* the padding too: rows compare as bytes */
        trimmed_row(rows[i].trim, R[i], cut[i].paired, cut[i].tau);
        rows[i].on_border = cut[i].pad;
    }
    const size_t mcap = std::min(cap, N);
    if (status && mcap) HIPCHK(h, copy_sync(h, status, G.tstatus.p, mcap, hipMemcpyDeviceToHost));
    if (d2 && mcap) HIPCHK(h, copy_sync(h, d2, G.td2.p, mcap * sizeof(float), hipMemcpyDeviceToHost));
    return PPP_OK;
}

int ppp_get_mesh_trimmed_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_mesh_trimmed_registration_params *mp, const double *T12,
                                            ppp_mesh_trimmed_registration_row *row, unsigned char *status, float *d2, size_t cap,
                                            ppp_registration_stats *stats)
{
    return mesh_trimmed_chain(h, m, mp, T12, false, row, row ? 1 : 0, status, d2, cap, stats);
}

int ppp_register_mesh_trimmed(ppp_handle h, ppp_trimesh m, const ppp_mesh_trimmed_registration_params *mp, const double *T0_12,
                              ppp_mesh_trimmed_registration_row *rows, size_t row_cap, unsigned char *status, float *d2, size_t cap,
                              ppp_registration_stats *stats)
{
    return mesh_trimmed_chain(h, m, mp, T0_12, true, rows, row_cap, status, d2, cap, stats);
}

} // extern "C"
