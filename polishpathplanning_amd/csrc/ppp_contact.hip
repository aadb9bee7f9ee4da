/*
 * ppp_contact.hip -- the contact queries of the C ABI (include/ppp_hip.h) on a finished pass or a resident cloud: coverage,
 * path coverage, path contacts, path removal, the dwell schedule, the feed schedule, the deviation map and its tiles, the registration, ppp_area2cloud, the principal curvatures, the contact field and its tiles, the regions,
 * their tiles and the merge.  The unit owns the kernels of ppp_contact.h, ppp_regions.h, ppp_removal.h, ppp_dwell.h, ppp_feed.h, ppp_deviation.h, ppp_deviation_tile.h, ppp_registration.h and ppp_trimmed.h; of the handle and the pass it
 * sees what ppp_handle.h declares.  Compiled with the engine's flags.
 */
#ifndef PPP_SINGLE_TU /* (a diagnostic build includes this file into the engine's unit) */
#define PPP_KERNELS_FOREIGN /* ppp_kernels.h, ppp_dynamic.h, ppp_compact.h: types and device helpers only -- their kernels are the engine's */
#endif
#include "ppp_handle.h"
#include "ppp_contact.h"
#include "ppp_regions.h"
#include "ppp_removal.h"
#include "ppp_dwell.h"
#include "ppp_feed.h"
#include "ppp_deviation.h"
#include "ppp_deviation_tile.h"
#include "ppp_registration.h"
#include "ppp_trimmed.h"
#include "ppp_registration_tile.h"
#include "ppp_trimmed_tile.h"
#include <cstring>

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

/* the kernels' views of the handle's slab index / normal field and of its knot tables, as they stand when the launch is made */
static ContactIndex contact_index(const ppp_handle h)
{
    return ContactIndex{h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_xmin.p, h->slab_xmax.p, h->normals4.p, h->ell_cs.p, h->slab_ytab.p};
}
static KnotTable knot_table(const ppp_handle h)
{
    return KnotTable{h->node_x.p, h->node_y.p, h->node_z.p, h->node_start.p, h->node_cnt.p, h->node_cap};
}

/* A finished pass with the dynamic adjustment left the normal field of THIS cloud and THESE parameters in normals4: every
   ppp_set_params and every cloud change plans again, which withdraws gen_done (a changed normal_radius included).  The
   contact queries then skip the launch; ppp_area2cloud, older than they are, builds the field every time and is left as it was. */
static bool pass_left_normals(const ppp_handle h) { return h->pass.gen_done() && h->P.dynamic_adjustment; }

/* behind index_ready: the Area2Cloud buffers and the normal field (a pass with the dynamic adjustment made it) */
static int contact_buffers(ppp_handle h)
{
    int rc = ensure_dynamic_buffers(h);
    if (rc) return rc;
    return pass_left_normals(h) ? PPP_OK : enqueue_normals(h);
}

/* What a pass did not build of what a contact query reads: the slab index (behind a window pass it keeps that pass's run
   state, gen_done with it, as every API mirror's does) and contact_buffers */
static int contact_prerequisites(ppp_handle h)
{
    int rc = index_ready(h, false);
    return rc ? rc : contact_buffers(h);
}

/* the opening of a query about the paths of a finished pass whose maps go by cloud index */
static int contact_query_begin(ppp_handle h, const char *what)
{
    int rc = ensure_ready(h, true, false);
    if (rc) return rc;
    rc = map_dev_err(h);
    if (rc) return rc;
    if (h->part_given)
        return fail(h, PPP_ERR_UNSUPPORTED, std::string(what) + ": the maps address the whole cloud: this handle holds a part (ppp_set_cloud_part)");
    return curvature_k_ok(h, h->P.curvature_k);
}

static PCovRange pcov_range(const ppp_handle h)
{
    return PCovRange{h->incl_lo, h->incl_hi, h->h_mn[0], h->h_mx[0], h->P.normal_radius, h->ranged ? 1 : 0};
}

/* the refusal word of the sample kernels: 1 wave_ball_leaves_range, 2 KnotTable::slice (or 2^24 samples on a slice), 4 the
   caps of k_pcon_offsets */
static int contact_refusal(ppp_handle h, const char *what, unsigned long long bits)
{
    const std::string w(what);
    if (bits & 2) return fail(h, PPP_ERR_HIP, w + ": a slice's knot table lies outside the node buffer");
    if (bits & 4) return fail(h, PPP_ERR_CAPACITY, w + ": more than 2^30 contact samples");
    if (bits & 1)
        return fail(h, PPP_ERR_CAPACITY, w + ": a contact search (Area2Cloud's neighbours, their normals or a ball) reaches beyond the indexed slice range: raise range_margin");
    return PPP_OK;
}

/* What both coverage calls share.  On the first question about a pass: the flags by cloud index (n16 uint4s: zero padding up to
   a multiple of 16 bytes) and the two result words zeroed, `mark` launches the balls (flags at C.flags.p, refusal word at
   C.count.p + 1), k_cov_count counts into C.count.p[0], one read brings both back.  Later questions answer from the result. */
static int flag_coverage(ppp_handle h, ppp_handle_s::FlagCoverage &C, const char *what, const std::function<int()> &mark, unsigned char *flags,
                         size_t cap, size_t *n, size_t *covered)
{
    const size_t N = h->n, n16 = (N + 15) / 16;
    if (C.serial != h->pass.serial()) {
        HIPCHK(h, C.flags.ensure(16 * std::max<size_t>(n16, 1))); HIPCHK(h, C.count.ensure(2));
        HIPCHK(h, hipMemsetAsync(C.flags.p, 0, 16 * std::max<size_t>(n16, 1), h->stream));
        HIPCHK(h, hipMemsetAsync(C.count.p, 0, 2 * sizeof(int), h->stream));
        int rc = mark();
        if (rc) return rc;
        if (n16)
            LAUNCH(h, "k_cov_count", k_cov_count, (unsigned)std::min<size_t>((n16 + COV_T - 1) / COV_T, 4 * (size_t)h->num_cus), COV_T, 0,
                   (const uint4 *)C.flags.p, (int)n16, C.count.p);
        int res[2] = {0, 0};
        HIPCHK(h, copy_sync(h, res, C.count.p, sizeof(res), hipMemcpyDeviceToHost));
        rc = contact_refusal(h, what, (unsigned)res[1]);
        if (rc) return rc;
        if (res[0] < 0 || (size_t)res[0] > N) return fail(h, PPP_ERR_HIP, std::string(what) + " count corrupt");
        C.covered = (size_t)res[0];
        C.serial = h->pass.serial();
    }
    if (n) *n = N;
    if (covered) *covered = C.covered;
    const size_t k = std::min(cap, N);
    if (flags && k) HIPCHK(h, copy_sync(h, flags, C.flags.p, k, hipMemcpyDeviceToHost));
    return PPP_OK;
}

int ppp_get_coverage(ppp_handle h, unsigned char *flags, size_t cap, size_t *n, size_t *covered)
{
    int rc = ensure_ready(h, true, false);
    if (rc) return rc;
    rc = map_dev_err(h);
    if (rc) return rc;
    if (h->P.walk != PPP_WALK_V1_CONTACT || !h->P.dynamic_adjustment || h->ranged || h->use_part || h->part_given)
        return fail(h, PPP_ERR_UNSUPPORTED, "coverage: only after a PPP_WALK_V1_CONTACT pass with dynamic_adjustment = 1 on a whole-cloud handle");
    auto balls = [h]() -> int { /* raw and adjusted paths of every slice, one launch */
        const int S = h->hmeta.S;
        if (S > 0)
            LAUNCH(h, "k_cov_balls", k_cov_balls, dim3((h->dyn_maxNB + DYN_WAVES - 1) / DYN_WAVES, S, 2), 64 * DYN_WAVES, 0, contact_index(h),
                   dyn_params(h), knot_table(h), h->dyn_raw_sc.p, h->dyn_maxNB, h->cov.flags.p);
        return PPP_OK;
    };
    return flag_coverage(h, h->cov, "coverage", balls, flags, cap, n, covered);
}

int ppp_get_path_coverage(ppp_handle h, unsigned char *flags, size_t cap, size_t *n, size_t *covered)
{
    int rc = contact_query_begin(h, "path coverage");
    if (rc) return rc;
    auto balls = [h]() -> int {
        int rc = contact_prerequisites(h);
        if (rc) return rc;
        const int S = h->hmeta.S, sb = std::min(h->sb, S), se = std::min(h->se, S);
        if (se <= sb) return PPP_OK;
        /* samples per slice of knots spanning the cloud's y range (the kernel strides past it where adjusted knots reach further) */
        const double yr = (double)h->h_mx[1] - (double)h->h_mn[1];
        const int nb = (int)std::min(65536.0, std::max(0.0, yr - 4) / (h->P.tool_radius / 4) + 4);
        for (int s0 = sb; s0 < se; s0 += 65535) /* (gridDim.y) */
            LAUNCH(h, "k_pcov_balls", k_pcov_balls, dim3((nb + DYN_WAVES - 1) / DYN_WAVES, std::min(se - s0, 65535)), 64 * DYN_WAVES, 0,
                   contact_index(h), dyn_params(h), knot_table(h), s0, pcov_range(h), h->pcov.flags.p, h->pcov.count.p + 1);
        return PPP_OK;
    };
    return flag_coverage(h, h->pcov, "path coverage", balls, flags, cap, n, covered);
}

/* The per-slice sample table of the last pass in h->pcon (off, tab, reach; k_pcon_offsets, k_pcon_samples), which the path
   contacts and the path removal both read: built on the first question about the pass, with what the pass left out
   (contact_prerequisites).  err: the device word the two kernels OR their refusals into, zeroed by the caller; the caller reads
   it back with its own results and only then calls pcon_table_accept, so a refused table is never reused. */
static int pcon_sample_table(ppp_handle h, const char *what, int *err)
{
    auto &C = h->pcon;
    if (C.tab_serial == h->pass.serial()) return PPP_OK;
    const int S = h->hmeta.S, sb = std::min(h->sb, S), se = std::min(h->se, S), nsl = std::max(se - sb, 0);
    int rc = contact_prerequisites(h);
    if (rc) return rc;
    C.tab_sb = sb; C.tab_nsl = nsl; C.tab_rows = 0;
    if (nsl <= 0) return PPP_OK;
    HIPCHK(h, C.off.ensure((size_t)nsl + 2));
    LAUNCH(h, "k_pcon_offsets", k_pcon_offsets, 1, PCON_T, 0, dyn_params(h), knot_table(h), sb, nsl, C.off.p, err);
    std::vector<int> off((size_t)nsl + 2);
    HIPCHK(h, copy_sync(h, off.data(), C.off.p, off.size() * sizeof(int), hipMemcpyDeviceToHost));
    rc = contact_refusal(h, what, (unsigned)off[nsl + 1]);
    if (rc) return rc;
    const int rows = off[nsl];
    int most = 0;
    for (int i = 0; i < nsl; ++i) most = std::max(most, off[i + 1] - off[i]);
    if (rows < 0 || most < 0) return fail(h, PPP_ERR_HIP, std::string(what) + ": sample table corrupt");
    if (rows > 0) {
        HIPCHK(h, C.tab.ensure((size_t)rows)); HIPCHK(h, C.reach.ensure(3 * (size_t)nsl));
        HIPCHK(h, hipMemsetAsync(C.reach.p, 0, 3 * (size_t)nsl * sizeof(unsigned), h->stream));
        const int gx = std::min((most + DYN_WAVES - 1) / DYN_WAVES, 16384);
        for (int s0 = 0; s0 < nsl; s0 += 65535) /* (gridDim.y) */
            LAUNCH(h, "k_pcon_samples", k_pcon_samples, dim3(gx, std::min(nsl - s0, 65535)), 64 * DYN_WAVES, 0, contact_index(h),
                   dyn_params(h), knot_table(h), C.off.p, sb, s0, pcov_range(h), C.tab.p, C.reach.p, err);
    }
    C.tab_rows = rows;
    return PPP_OK;
}
static void pcon_table_accept(ppp_handle h) { h->pcon.tab_serial = h->pass.serial(); }

int ppp_get_path_contacts(ppp_handle h, unsigned int *counts, int *first_slice, int *last_slice, size_t cap, ppp_contact_stats *stats)
{
    int rc = contact_query_begin(h, "path contacts");
    if (rc) return rc;
    const size_t N = h->n;
    auto &C = h->pcon;
    if (C.serial != h->pass.serial()) { /* first question about this pass */
        const size_t N1 = std::max<size_t>(N, 1);
        HIPCHK(h, C.counts.ensure(N1)); HIPCHK(h, C.first.ensure(N1)); HIPCHK(h, C.last.ensure(N1));
        HIPCHK(h, C.acc.ensure(70));
        HIPCHK(h, hipMemsetAsync(C.counts.p, 0, N1 * sizeof(unsigned), h->stream));
        HIPCHK(h, hipMemsetAsync(C.first.p, 0xff, N1 * sizeof(int), h->stream));
        HIPCHK(h, hipMemsetAsync(C.last.p, 0xff, N1 * sizeof(int), h->stream));
        HIPCHK(h, hipMemsetAsync(C.acc.p, 0, 70 * sizeof(unsigned long long), h->stream));
        int *err = (int *)(C.acc.p + 69);
        rc = pcon_sample_table(h, "path contacts", err);
        if (rc) return rc;
        if (C.tab_rows > 0) /* one thread per indexed point (at most N of them), PCON_T a round */
            LAUNCH(h, "k_pcon_points", k_pcon_points, (unsigned)std::min<size_t>((N + PCON_T - 1) / PCON_T, 1u << 20), PCON_T, 0,
                   h->meta.p, h->sorted4.p, C.tab.p, C.off.p, C.reach.p, C.tab_sb, C.tab_nsl, C.counts.p, C.first.p, C.last.p);
        LAUNCH(h, "k_pcon_stats", k_pcon_stats, (unsigned)std::min<size_t>((N1 + PCON_T - 1) / PCON_T, 2 * (size_t)h->num_cus), PCON_T, 0,
               C.counts.p, C.first.p, C.last.p, (int)N, err, C.acc.p);
        unsigned long long acc[69];
        HIPCHK(h, copy_sync(h, acc, C.acc.p, sizeof(acc), hipMemcpyDeviceToHost));
        rc = contact_refusal(h, "path contacts", acc[68]);
        if (rc) return rc;
        if (acc[64] > N || acc[65] > acc[64]) return fail(h, PPP_ERR_HIP, "path contacts: statistics corrupt");
        pcon_table_accept(h);
        ppp_contact_stats st = {};
        st.n = N; st.covered = (size_t)acc[64]; st.multi_slice = (size_t)acc[65];
        st.total = acc[66]; st.max_count = (unsigned)acc[67];
        st.hist[0] = N - st.covered;
        for (int b = 1; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[b];
        C.stats = st;
        C.serial = h->pass.serial();
    }
    if (stats) *stats = C.stats;
    const size_t k = std::min(cap, N);
    if (counts && k) HIPCHK(h, copy_sync(h, counts, C.counts.p, k * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (first_slice && k) HIPCHK(h, copy_sync(h, first_slice, C.first.p, k * sizeof(int), hipMemcpyDeviceToHost));
    if (last_slice && k) HIPCHK(h, copy_sync(h, last_slice, C.last.p, k * sizeof(int), hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* the double whose bit pattern an accumulator word holds (k_prem_range, k_dwell_stats, k_feed_stats) */
static double bits_as_double(unsigned long long k) { double d; memcpy(&d, &k, sizeof(d)); return d; }

/* The partition of a map of N entries for a fixed-order sum (B.46, block_tree_sum): workgroup g of grid takes [g per, (g + 1) per);
   the host adds the workgroups' parts in order */
struct MapParts {
    int grid, per;
    MapParts(const ppp_handle h, size_t N)
        : grid((int)std::max<size_t>(1, std::min<size_t>((N + PCON_T - 1) / PCON_T, 2 * (size_t)h->num_cus))), per((int)((N + grid - 1) / grid)) {}
};

static int removal_profile_ok(ppp_handle h, const char *what, int profile)
{
    if (profile != PPP_REMOVAL_FLAT && profile != PPP_REMOVAL_PARABOLIC && profile != PPP_REMOVAL_HERTZ)
        return fail(h, PPP_ERR_ARG, std::string(what) + ": unknown profile (PPP_REMOVAL_FLAT, _PARABOLIC or _HERTZ)");
    return PPP_OK;
}

/* a call that needs every slice of the walk on one handle refuses a slice-range handle */
static int whole_walk_only(ppp_handle h, const char *what, const char *why)
{
    if (h->P.slice_begin != 0 || h->P.slice_end != 0 || h->ranged || h->use_part) return fail(h, PPP_ERR_UNSUPPORTED, std::string(what) + ": " + why);
    return PPP_OK;
}

/* The point walk with the profile's weight over the handle's sample table: map[cloud index] = the sum of w * ds over the balls
   that hold the point, held flags beside it.  The one place that picks k_prem_points's instantiation. */
static int launch_prem_points(ppp_handle h, int profile, const double *ds, double *map)
{
    const auto &T = h->pcon;
    auto points = profile == PPP_REMOVAL_FLAT ? k_prem_points<PPP_REMOVAL_FLAT>
                : profile == PPP_REMOVAL_PARABOLIC ? k_prem_points<PPP_REMOVAL_PARABOLIC> : k_prem_points<PPP_REMOVAL_HERTZ>;
    LAUNCH(h, "k_prem_points", points, (unsigned)std::min<size_t>((h->n + PCON_T - 1) / PCON_T, 1u << 20), PCON_T, 0, h->meta.p, h->sorted4.p,
           T.tab.p, ds, T.off.p, T.reach.p, T.tab_nsl, map, h->prem.held.p);
    return PPP_OK;
}

/* the transposed walk of every row of the handle's sample table (k_dwell_back): num, and den where with_den.  The one place
   that picks k_dwell_back's instantiation. */
static int launch_dwell_back(ppp_handle h, int profile, bool with_den, const double *g, long long *num, long long *den)
{
    const auto &T = h->pcon;
    auto form = [with_den](auto with, auto without) { return with_den ? with : without; };
    auto back = profile == PPP_REMOVAL_FLAT ? form(k_dwell_back<PPP_REMOVAL_FLAT, true>, k_dwell_back<PPP_REMOVAL_FLAT, false>)
              : profile == PPP_REMOVAL_PARABOLIC ? form(k_dwell_back<PPP_REMOVAL_PARABOLIC, true>, k_dwell_back<PPP_REMOVAL_PARABOLIC, false>)
                                                 : form(k_dwell_back<PPP_REMOVAL_HERTZ, true>, k_dwell_back<PPP_REMOVAL_HERTZ, false>);
    LAUNCH(h, "k_dwell_back", back, (unsigned)((T.tab_rows + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, contact_index(h), T.tab.p, T.tab_rows, g,
           num, den);
    return PPP_OK;
}

/* The predicted removal: the sample table of the path contacts (shared with that call when the handle holds
   one for the pass), the path length of every sample (k_prem_ds, once per pass), the point walk with the profile's weight
   (k_prem_points) and the statistics in two phases (k_prem_range, k_prem_stats); kept per (pass, profile). */
int ppp_get_path_removal(ppp_handle h, int profile, double *removal, size_t cap, ppp_removal_stats *stats)
{
    int rc = contact_query_begin(h, "path removal");
    if (rc) return rc;
    rc = removal_profile_ok(h, "path removal", profile);
    if (rc) return rc;
    const size_t N = h->n;
    auto &R = h->prem;
    auto &M = R.slot[profile];
    const auto &T = h->pcon;
    if (M.serial != h->pass.serial()) { /* first question about this pass with this profile */
        const size_t N1 = std::max<size_t>(N, 1);
        const MapParts parts(h, N);
        const int grid = parts.grid, per = parts.per;
        HIPCHK(h, M.map.ensure(N1)); HIPCHK(h, R.held.ensure(N1));
        HIPCHK(h, R.acc.ensure(PREM_ACC_WORDS)); HIPCHK(h, R.psum.ensure(2 * (size_t)grid));
        HIPCHK(h, hipMemsetAsync(M.map.p, 0, N1 * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(R.held.p, 0, N1, h->stream));
        HIPCHK(h, hipMemsetAsync(R.acc.p, 0, PREM_ACC_WORDS * sizeof(unsigned long long), h->stream));
        rc = pcon_sample_table(h, "path removal", (int *)(R.acc.p + PREM_ACC_ERR));
        if (rc) return rc;
        const bool new_ds = R.ds_serial != h->pass.serial();
        if (T.tab_rows > 0) {
            if (new_ds) {
                HIPCHK(h, R.ds.ensure((size_t)T.tab_rows)); HIPCHK(h, R.slice_len.ensure((size_t)T.tab_nsl));
                LAUNCH(h, "k_prem_ds", k_prem_ds, (unsigned)T.tab_nsl, PCON_T, 0, T.tab.p, T.off.p, R.ds.p, R.slice_len.p);
            }
            rc = launch_prem_points(h, profile, R.ds.p, M.map.p);
            if (rc) return rc;
        }
        LAUNCH(h, "k_prem_range", k_prem_range, (unsigned)grid, PCON_T, 0, M.map.p, R.held.p, (int)N, R.acc.p);
        LAUNCH(h, "k_prem_stats", k_prem_stats, (unsigned)grid, PCON_T, 0, M.map.p, R.held.p, (int)N, per, R.acc.p, R.acc.p + PREM_ACC_BINS,
               R.psum.p, R.psum.p + grid);
        unsigned long long acc[PREM_ACC_WORDS];
        std::vector<double> psum(2 * (size_t)grid), len;
        HIPCHK(h, copy_sync(h, acc, R.acc.p, sizeof(acc), hipMemcpyDeviceToHost));
        rc = contact_refusal(h, "path removal", (unsigned)acc[PREM_ACC_ERR]);
        if (rc) return rc;
        if (acc[0] > N) return fail(h, PPP_ERR_HIP, "path removal: statistics corrupt");
        pcon_table_accept(h);
        HIPCHK(h, copy_sync(h, psum.data(), R.psum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (new_ds) { /* the slices' lengths in slice order */
            R.path_length = 0.0;
            if (T.tab_rows > 0) {
                len.resize((size_t)T.tab_nsl);
                HIPCHK(h, copy_sync(h, len.data(), R.slice_len.p, len.size() * sizeof(double), hipMemcpyDeviceToHost));
                for (double v : len) R.path_length += v;
            }
            R.ds_serial = h->pass.serial();
        }
        ppp_removal_stats st = {};
        st.n = N; st.touched = (size_t)acc[0];
        st.max_removal = st.touched ? bits_as_double(acc[1]) : (double)NAN; st.min_removal = st.touched ? bits_as_double(~acc[2]) : (double)NAN;
        for (int g = 0; g < grid; ++g) { st.sum += psum[(size_t)g]; st.sum_sq += psum[(size_t)grid + g]; }
        st.path_length = R.path_length;
        for (int b = 0; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[PREM_ACC_BINS + b];
        M.stats = st;
        M.serial = h->pass.serial();
    }
    if (stats) *stats = M.stats;
    const size_t k = std::min(cap, N);
    if (removal && k) HIPCHK(h, copy_sync(h, removal, M.map.p, k * sizeof(double), hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* The dwell schedule: the unit-feed map, the sample table, ds and the held flags come from
   ppp_get_path_removal's own call (built if the handle does not hold them, refused as it refuses); then every round's kernels
   back to back on the stream -- forward (k_dwell_scale + k_prem_points; the first round reads the unit-feed map, which IS the
   forward pass at t = 1), k_dwell_ratio, k_dwell_back, k_dwell_update -- the last forward pass, the residuals and the factors'
   statistics, and one wait.  Kept per (pass, profile, iterations, bounds) when there is no target. */
int ppp_get_path_dwell(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,
                       ppp_dwell_row *rows, size_t row_cap, double *removal, size_t cap, ppp_dwell_stats *stats)
{
    int rc = contact_query_begin(h, "path dwell");
    if (rc) return rc;
    rc = removal_profile_ok(h, "path dwell", profile);
    if (rc) return rc;
    if (iterations < 1 || iterations > 64) return fail(h, PPP_ERR_ARG, "path dwell: iterations must lie in [1, 64]");
    if (!(std::isfinite(dwell_min) && std::isfinite(dwell_max) && dwell_min > 0.0 && dwell_min <= 1.0 && dwell_max >= 1.0))
        return fail(h, PPP_ERR_ARG, "path dwell: the bounds must be finite with 0 < dwell_min <= 1 <= dwell_max");
    rc = whole_walk_only(h, "path dwell", "neighbouring slice ranges share the points of their overlap bands: a slice-range handle cannot solve alone");
    if (rc) return rc;
    const size_t N = h->n;
    auto &D = h->dwell;
    const bool reuse = !target && D.valid && D.serial == h->pass.serial() && D.profile == profile && D.iterations == iterations &&
                       D.dmin == dwell_min && D.dmax == dwell_max;
    if (!reuse) {
        D.valid = false;
        ppp_removal_stats rs = {};
        rc = ppp_get_path_removal(h, profile, nullptr, 0, &rs);
        if (rc) return rc;
        auto &R = h->prem;
        const auto &M = R.slot[profile];
        const auto &T = h->pcon;
        const int nrow = T.tab_rows, nsl = T.tab_nsl;
        const size_t N1 = std::max<size_t>(N, 1), R1 = (size_t)std::max(nrow, 1), touched = rs.touched;
        const MapParts parts(h, N);
        const int grid = parts.grid, per = parts.per;
        const unsigned gn = (unsigned)((N1 + PCON_T - 1) / PCON_T), gr = (unsigned)((R1 + PCON_T - 1) / PCON_T);
        HIPCHK(h, D.t.ensure(R1)); HIPCHK(h, D.dst.ensure(R1)); HIPCHK(h, D.num.ensure(R1)); HIPCHK(h, D.den.ensure(R1));
        HIPCHK(h, D.g.ensure(N1)); HIPCHK(h, D.map.ensure(N1)); HIPCHK(h, D.psum.ensure(2 * (size_t)grid));
        HIPCHK(h, D.acc.ensure(PREM_ACC_WORDS));
        double level = touched ? rs.sum / (double)touched : (double)NAN;
        const double *dtarget = nullptr;
        if (target) {
            if (touched) { /* the entries the solve reads */
                std::vector<unsigned char> held(N);
                HIPCHK(h, copy_sync(h, held.data(), R.held.p, N, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < N; ++i)
                    if (held[i] && !(target[i] >= 0.0 && std::isfinite(target[i])))
                        return fail(h, PPP_ERR_ARG, "path dwell: the target must be finite and >= 0 at every touched point");
            }
            HIPCHK(h, D.target.ensure(N1));
            if (N) HIPCHK(h, copy_sync(h, D.target.p, target, N * sizeof(double), hipMemcpyHostToDevice));
            dtarget = D.target.p;
            if (touched) { /* L = the mean of T over the touched points, as k_prem_stats adds a map (its bins: all in bin 0, not read) */
                HIPCHK(h, hipMemsetAsync(D.acc.p, 0, PREM_ACC_WORDS * sizeof(unsigned long long), h->stream));
                LAUNCH(h, "k_prem_stats", k_prem_stats, (unsigned)grid, PCON_T, 0, D.target.p, R.held.p, (int)N, per, D.acc.p, D.acc.p + PREM_ACC_BINS,
                       D.psum.p, D.psum.p + grid);
                std::vector<double> ps((size_t)grid);
                HIPCHK(h, copy_sync(h, ps.data(), D.psum.p, ps.size() * sizeof(double), hipMemcpyDeviceToHost));
                double sum = 0.0;
                for (double v : ps) sum += v;
                level = sum / (double)touched;
            }
        }
        const bool walk = nrow > 0 && touched > 0, solve = walk && level > 0.0;
        HIPCHK(h, hipMemsetAsync(D.map.p, 0, N1 * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(D.acc.p, 0, 4 * sizeof(unsigned long long), h->stream));
        std::vector<double> tv((size_t)nrow, 1.0), dsv((size_t)nrow);
        if (walk) {
            HIPCHK(h, hipMemsetAsync(D.g.p, 0, N1 * sizeof(double), h->stream));
            HIPCHK(h, copy_sync(h, D.t.p, tv.data(), tv.size() * sizeof(double), hipMemcpyHostToDevice));
            auto forward = [&]() -> int { /* D.map = the removal the factors predict */
                LAUNCH(h, "k_dwell_scale", k_dwell_scale, gr, PCON_T, 0, R.ds.p, D.t.p, nrow, D.dst.p);
                return launch_prem_points(h, profile, D.dst.p, D.map.p);
            };
            auto back = [&](bool with_den) { return launch_dwell_back(h, profile, with_den, D.g.p, D.num.p, D.den.p); };
            const double *cur = M.map.p; /* the forward pass at t = 1 */
            if (solve) LAUNCH(h, "k_dwell_resid", k_dwell_resid, (unsigned)grid, PCON_T, 0, cur, dtarget, level, R.held.p, (int)N, per, D.psum.p);
            for (int it = 0; solve && it < iterations; ++it) { /* no host wait in here */
                if (it > 0) { rc = forward(); if (rc) return rc; cur = D.map.p; }
                LAUNCH(h, "k_dwell_ratio", k_dwell_ratio, gn, PCON_T, 0, cur, dtarget, level, R.held.p, (int)N, D.g.p);
                rc = back(it == 0);
                if (rc) return rc;
                LAUNCH(h, "k_dwell_update", k_dwell_update, gr, PCON_T, 0, D.num.p, D.den.p, nrow, dwell_min, dwell_max, D.t.p);
            }
            if (!solve) { rc = back(true); if (rc) return rc; } /* den alone: which rows hold something */
            rc = forward();
            if (rc) return rc;
            if (solve) LAUNCH(h, "k_dwell_resid", k_dwell_resid, (unsigned)grid, PCON_T, 0, D.map.p, dtarget, level, R.held.p, (int)N, per, D.psum.p + grid);
            LAUNCH(h, "k_dwell_stats", k_dwell_stats, (unsigned)std::min<size_t>(gr, 2 * (size_t)h->num_cus), PCON_T, 0, D.t.p, D.den.p, nrow, dwell_min,
                   dwell_max, D.acc.p);
        }
        unsigned long long acc[4];
        std::vector<double> psum(2 * (size_t)grid, 0.0);
        HIPCHK(h, copy_sync(h, acc, D.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
        if (solve) HIPCHK(h, copy_sync(h, psum.data(), D.psum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (acc[0] > (size_t)nrow || acc[1] > (size_t)nrow) return fail(h, PPP_ERR_HIP, "path dwell: statistics corrupt");
        D.rows.assign((size_t)nrow, ppp_dwell_row{});
        double wsum = 0.0;
        if (nrow > 0) {
            std::vector<float4> tab((size_t)nrow);
            std::vector<int> off((size_t)nsl + 1);
            if (walk) HIPCHK(h, copy_sync(h, tv.data(), D.t.p, tv.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(h, copy_sync(h, dsv.data(), R.ds.p, dsv.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(h, copy_sync(h, tab.data(), T.tab.p, tab.size() * sizeof(float4), hipMemcpyDeviceToHost));
            HIPCHK(h, copy_sync(h, off.data(), T.off.p, off.size() * sizeof(int), hipMemcpyDeviceToHost));
            if (off[0] != 0 || off[(size_t)nsl] != nrow) return fail(h, PPP_ERR_HIP, "path dwell: sample table corrupt");
            for (int i = 0; i < nsl; ++i) {
                if (off[(size_t)i + 1] < off[(size_t)i]) return fail(h, PPP_ERR_HIP, "path dwell: sample table corrupt");
                double len = 0.0; /* the slice's scaled lengths in sample order, the slices in order: path_length's scheme */
                for (int j = off[(size_t)i]; j < off[(size_t)i + 1]; ++j) {
                    const float4 &q = tab[(size_t)j];
                    const double scaled = dsv[(size_t)j] * tv[(size_t)j];
                    len += scaled;
                    D.rows[(size_t)j] = ppp_dwell_row{T.tab_sb + i, q.x, q.y, q.z, std::sqrt(q.w), dsv[(size_t)j], tv[(size_t)j]};
                }
                wsum += len;
            }
        }
        ppp_dwell_stats st = {};
        st.n = N; st.touched = touched; st.rows = (size_t)nrow; st.at_min = (size_t)acc[0]; st.at_max = (size_t)acc[1];
        st.iterations = iterations; st.level = level;
        st.residual_before = st.residual_after = (double)NAN;
        if (solve) {
            double before = 0.0, after = 0.0;
            for (int g = 0; g < grid; ++g) { before += psum[(size_t)g]; after += psum[(size_t)grid + g]; }
            st.residual_before = std::sqrt(before / (double)touched); st.residual_after = std::sqrt(after / (double)touched);
        }
        st.max_dwell = acc[3] ? bits_as_double(acc[2]) : (double)NAN; st.min_dwell = acc[3] ? bits_as_double(~acc[3]) : (double)NAN;
        st.path_length = rs.path_length; st.time_factor = wsum / rs.path_length;
        D.stats = st;
        D.serial = h->pass.serial(); D.profile = profile; D.iterations = iterations; D.dmin = dwell_min; D.dmax = dwell_max;
        D.valid = !target;
    }
    if (stats) *stats = D.stats;
    const size_t kr = std::min(row_cap, D.rows.size()), k = std::min(cap, N);
    if (rows && kr) memcpy(rows, D.rows.data(), kr * sizeof(ppp_dwell_row));
    if (removal && k) HIPCHK(h, copy_sync(h, removal, D.map.p, k * sizeof(double), hipMemcpyDeviceToHost));
    return PPP_OK;
}

void ppp_default_feed_params(ppp_feed_params *fp)
{
    if (!fp) return;
    fp->feed = 20.0; fp->feed_max = 30.0; fp->accel = 100.0; fp->end_feed = 0.0; fp->link_feed = 100.0;
}

/* The feed schedule: the dwell rows come from ppp_get_path_dwell's own call (built if the handle does not hold
   them, refused as it refuses), the list from the last getPath (its stage list gathered into list order if a window pass left
   it in slots).  The kept slices' offsets into the list and into the rows are made on the host from the counts; then
   k_feed_map, k_feed_scan, k_feed_env, k_feed_time and its two followers and k_feed_stats back to back on the stream, and one
   wait.  Kept per (pass, profile, iterations, bounds, feed parameters) when there is no target. */
int ppp_get_path_feed(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,
                      const ppp_feed_params *fp, ppp_feed_row *rows, size_t cap, ppp_feed_stats *stats)
{
    int rc = contact_query_begin(h, "path feed");
    if (rc) return rc;
    if (!fp) return fail(h, PPP_ERR_ARG, "path feed: no feed parameters");
    if (!(std::isfinite(fp->feed) && fp->feed > 0.0)) return fail(h, PPP_ERR_ARG, "path feed: feed must be finite and > 0");
    if (!(std::isfinite(fp->feed_max) && fp->feed_max >= fp->feed)) return fail(h, PPP_ERR_ARG, "path feed: feed_max must be finite and >= feed");
    if (!(fp->accel > 0.0)) return fail(h, PPP_ERR_ARG, "path feed: accel must be > 0 (+INFINITY: no limit)");
    if (!std::isfinite(fp->end_feed)) return fail(h, PPP_ERR_ARG, "path feed: end_feed must be finite (< 0: no cap at a slice's ends)");
    if (!(std::isfinite(fp->link_feed) && fp->link_feed > 0.0)) return fail(h, PPP_ERR_ARG, "path feed: link_feed must be finite and > 0");
    rc = whole_walk_only(h, "path feed", "the dwell schedule it times cannot be solved on a slice-range handle");
    if (rc) return rc;
    if (h->aligned)
        return fail(h, PPP_ERR_UNSUPPORTED, "path feed: under ppp_trans2center the list's points are in the scanner's frame and the dwell rows in the aligned one");
    rc = ensure_ready(h, true, true); /* the waypoints must exist */
    if (rc) return rc;
    auto &F = h->feed;
    const ppp_feed_params P = *fp;
    const bool reuse = !target && F.valid && F.serial == h->pass.serial() && F.profile == profile && F.iterations == iterations &&
                       F.dmin == dwell_min && F.dmax == dwell_max && memcmp(&F.fp, &P, sizeof(P)) == 0;
    if (!reuse) {
        F.valid = false;
        ppp_dwell_stats dst = {};
        rc = ppp_get_path_dwell(h, profile, target, iterations, dwell_min, dwell_max, nullptr, 0, nullptr, 0, &dst);
        if (rc) return rc;
        const std::vector<ppp_dwell_row> &DR = h->dwell.rows;
        size_t Wl = 0, nkl = 0;
        rc = ppp_get_stage(h, PPP_STAGE_WP_XYZ, nullptr, 0, &Wl); /* the list order of wp_xyz */
        if (rc) return rc;
        rc = ppp_get_waypoint_counts(h, nullptr, 0, &nkl);
        if (rc) return rc;
        if (Wl > 0x7ffffff0u || nkl > 0x7ffffff0u) return fail(h, PPP_ERR_CAPACITY, "path feed: more than 2^31 waypoints");
        const int W = (int)Wl, nk = (int)nkl, first_kept = h->hmeta.first_kept;
        std::vector<int> off((size_t)nk + 1, 0), rowoff((size_t)nk + 1, 0);
        if (nk) { rc = ppp_get_waypoint_counts(h, off.data() + 1, nkl, &nkl); if (rc) return rc; }
        std::vector<int2> tiles;
        size_t slices = 0;
        for (int k = 0; k < nk; ++k) {
            const int m = off[(size_t)k + 1];
            if (m < 0 || m > W - off[(size_t)k]) return fail(h, PPP_ERR_HIP, "path feed: waypoint counts corrupt");
            off[(size_t)k + 1] = off[(size_t)k] + m;
            slices += m > 0;
            for (int i0 = 0; i0 < m; i0 += FEED_TILE) tiles.push_back(make_int2(k, i0));
        }
        if (off[(size_t)nk] != W) return fail(h, PPP_ERR_HIP, "path feed: waypoint counts corrupt");
        /* the rows come in (slice, sample) order: slice k's are those of walk slice first_kept + k */
        const size_t R = DR.size();
        std::vector<float> ry(R);
        std::vector<double> rt(R);
        {
            size_t j = 0;
            for (int k = 0; k < nk; ++k) {
                while (j < R && DR[j].slice < first_kept + k) ++j;
                rowoff[(size_t)k] = (int)j;
            }
            while (j < R && DR[j].slice < first_kept + nk) ++j;
            rowoff[(size_t)nk] = (int)j;
            for (j = 0; j < R; ++j) { ry[j] = DR[j].y; rt[j] = DR[j].dwell; }
        }
        F.host_rows.assign((size_t)W, ppp_feed_row{});
        unsigned long long acc[FEED_ACC_WORDS] = {};
        if (W > 0) {
            const size_t W1 = (size_t)W, K1 = (size_t)nk, R1 = std::max<size_t>(R, 1);
            HIPCHK(h, F.off.ensure(K1 + 1)); HIPCHK(h, F.rowoff.ensure(K1 + 1)); HIPCHK(h, F.tiles.ensure(tiles.size()));
            HIPCHK(h, F.ry.ensure(R1)); HIPCHK(h, F.rt.ensure(R1)); HIPCHK(h, F.cap.ensure(W1)); HIPCHK(h, F.D.ensure(W1));
            HIPCHK(h, F.tloc.ensure(W1)); HIPCHK(h, F.rec.ensure(W1)); HIPCHK(h, F.rows.ensure(W1)); HIPCHK(h, F.linkD.ensure(K1));
            HIPCHK(h, F.linkT.ensure(K1)); HIPCHK(h, F.slice_len.ensure(K1)); HIPCHK(h, F.slice_t.ensure(K1)); HIPCHK(h, F.acc.ensure(FEED_ACC_WORDS));
            HIPCHK(h, copy_sync(h, F.off.p, off.data(), (K1 + 1) * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(h, copy_sync(h, F.rowoff.p, rowoff.data(), (K1 + 1) * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(h, copy_sync(h, F.tiles.p, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice));
            if (R) {
                HIPCHK(h, copy_sync(h, F.ry.p, ry.data(), R * sizeof(float), hipMemcpyHostToDevice));
                HIPCHK(h, copy_sync(h, F.rt.p, rt.data(), R * sizeof(double), hipMemcpyHostToDevice));
            }
            HIPCHK(h, hipMemsetAsync(F.linkD.p, 0, K1 * sizeof(long long), h->stream));
            HIPCHK(h, hipMemsetAsync(F.linkT.p, 0, K1 * sizeof(long long), h->stream));
            HIPCHK(h, hipMemsetAsync(F.acc.p, 0, FEED_ACC_WORDS * sizeof(unsigned long long), h->stream));
            const unsigned gw = (unsigned)((W1 + PCON_T - 1) / PCON_T);
            LAUNCH(h, "k_feed_map", k_feed_map, gw, PCON_T, 0, h->wp_xyz.p, F.off.p, nk, W, first_kept, F.rowoff.p, F.ry.p, F.rt.p, P.feed, P.feed_max,
                   P.end_feed, P.link_feed, F.rows.p, F.cap.p, F.D.p, F.linkD.p, F.linkT.p);
            LAUNCH(h, "k_feed_scan", k_feed_scan, (unsigned)nk, PCON_T, 0, F.off.p, F.D.p, F.cap.p, F.rec.p, F.slice_len.p);
            LAUNCH(h, "k_feed_env", k_feed_env, (unsigned)tiles.size(), FEED_TILE, 0, F.tiles.p, F.off.p, F.rec.p, P.accel, F.rows.p);
            LAUNCH(h, "k_feed_time", k_feed_time, (unsigned)nk, PCON_T, 0, F.off.p, F.rows.p, F.D.p, F.linkT.p, P.accel, F.tloc.p, F.slice_t.p);
            LAUNCH(h, "k_feed_time_slices", k_feed_time_slices, 1, PCON_T, 0, nk, F.slice_t.p, F.linkT.p, F.slice_len.p, F.linkD.p, F.acc.p);
            LAUNCH(h, "k_feed_time_rows", k_feed_time_rows, gw, PCON_T, 0, W, first_kept, F.tloc.p, F.slice_t.p, F.rows.p);
            LAUNCH(h, "k_feed_stats", k_feed_stats, std::min<unsigned>(gw, 2u * (unsigned)h->num_cus), PCON_T, 0, F.rows.p, W, F.acc.p);
            HIPCHK(h, copy_sync(h, acc, F.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
            HIPCHK(h, copy_sync(h, F.host_rows.data(), F.rows.p, W1 * sizeof(ppp_feed_row), hipMemcpyDeviceToHost));
            if (acc[0] + acc[1] + acc[2] + acc[3] != (unsigned long long)W) return fail(h, PPP_ERR_HIP, "path feed: statistics corrupt");
        }
        auto fixed = [](unsigned long long k, double one) { return (double)(long long)k * (1.0 / one); };
        ppp_feed_stats st = {};
        st.W = (size_t)W; st.slices = slices;
        st.by_dwell = (size_t)acc[FEED_ACC_LIMIT]; st.by_feed_max = (size_t)acc[FEED_ACC_LIMIT + 1]; st.by_end = (size_t)acc[FEED_ACC_LIMIT + 2];
        st.by_accel = (size_t)acc[FEED_ACC_LIMIT + 3];
        st.max_feed = W ? bits_as_double(acc[FEED_ACC_MAX]) : (double)NAN; st.min_feed = W ? bits_as_double(~acc[FEED_ACC_NMIN]) : (double)NAN;
        st.path_length = fixed(acc[FEED_ACC_PATH], FEED_LEN_FIXED); st.link_length = fixed(acc[FEED_ACC_LINK], FEED_LEN_FIXED);
        st.duration = fixed(acc[FEED_ACC_DUR], FEED_TIME_FIXED); st.duration_links = fixed(acc[FEED_ACC_DUR_LINKS], FEED_TIME_FIXED);
        st.duration_nominal = st.path_length / P.feed;
        F.stats = st;
        F.serial = h->pass.serial(); F.profile = profile; F.iterations = iterations; F.dmin = dwell_min; F.dmax = dwell_max; F.fp = P;
        F.valid = !target;
    }
    if (stats) *stats = F.stats;
    const size_t k = std::min(cap, F.host_rows.size());
    if (rows && k) memcpy(rows, F.host_rows.data(), k * sizeof(ppp_feed_row));
    return PPP_OK;
}

int ppp_area2cloud(ppp_handle h, const double *pts_xyz, size_t k, int key, float *out3)
{
    int rc = index_ready(h, false); /* complete index: slabs beyond the LDS capacity go through the arena pass first */
    if (rc) return rc;
    if (!k) return PPP_OK;
    if (!pts_xyz || !out3 || (key != 0 && key != 1)) return fail(h, PPP_ERR_ARG, "bad arguments");
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    rc = ensure_dynamic_buffers(h);
    if (rc) return rc;
    rc = enqueue_normals(h);
    if (rc) return rc;
    HIPCHK(h, h->scratch.ensure(k * 36 + 64));
    double *dq = (double *)h->scratch.p;
    float *dout = (float *)(dq + 3 * k);
    HIPCHK(h, hipMemcpyAsync(dq, pts_xyz, k * 24, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "k_area2cloud_api", k_area2cloud_api, (unsigned)((k + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, contact_index(h), dyn_params(h),
           dq, (int)k, key, dout);
    HIPCHK(h, hipMemcpyAsync(out3, dout, k * 12, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PPP_OK;
}

int ppp_principal_curvatures_at(ppp_handle h, const float *q_xyz, size_t k, float *out5)
{
    int rc = index_ready(h, false); /* complete index: slabs beyond the LDS capacity go through the arena pass first */
    if (rc) return rc;
    if (!k) return PPP_OK;
    if (!q_xyz || !out5 || k > 0x7fffffffu / 8) return fail(h, PPP_ERR_ARG, "bad arguments");
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    rc = contact_buffers(h);
    if (rc) return rc;
    HIPCHK(h, h->scratch.ensure(k * 32 + 64));
    float *dq = (float *)h->scratch.p, *dout = dq + 3 * k;
    HIPCHK(h, hipMemcpyAsync(dq, q_xyz, k * 12, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "k_field_waves", k_field_waves, (unsigned)((k + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, contact_index(h), dyn_params(h),
           dq, (int)k, dout, (float *)nullptr);
    HIPCHK(h, hipMemcpyAsync(out5, dout, k * 20, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PPP_OK;
}

/* the opening of the field and region calls: a handle, on its device, that holds a cloud and holds all of it.  what: the call's
   name in the refusal, why: what a part cannot give it */
static int whole_cloud_begin(ppp_handle h, const char *what, const char *why)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->have_cloud) return fail(h, PPP_ERR_ARG, "no cloud set");
    if (h->part_given) return fail(h, PPP_ERR_UNSUPPORTED, std::string(what) + ": " + why + ": this handle holds a part (ppp_set_cloud_part)");
    return PPP_OK;
}

/* the parameters a contact field depends on */
static bool same_contact_params(const ppp_params &P, const ppp_params &F)
{
    return P.tool_radius == F.tool_radius && P.depth == F.depth && P.toolthickness == F.toolthickness && P.curvature_k == F.curvature_k &&
           P.normal_radius == F.normal_radius && P.change_range == F.change_range;
}

/* the statistics of a stored half-width map for one min_width (k_field_stats): hw = N half widths by cloud index */
static int field_statistics(ppp_handle h, const float *hw, DevBuf<unsigned long long> &dacc, DevBuf<double> &dpsum, float min_width,
                            ppp_contact_field_stats &st)
{
    const size_t N = h->n;
    const MapParts parts(h, N);
    const int grid = parts.grid, per = parts.per;
    HIPCHK(h, dacc.ensure(68)); HIPCHK(h, dpsum.ensure((size_t)grid));
    HIPCHK(h, hipMemsetAsync(dacc.p, 0, 68 * sizeof(unsigned long long), h->stream));
    LAUNCH(h, "k_field_stats", k_field_stats, (unsigned)grid, PCON_T, 0, hw, (int)N, per, h->P.tool_radius, min_width, dacc.p, dpsum.p);
    unsigned long long acc[68];
    std::vector<double> psum((size_t)grid);
    HIPCHK(h, copy_sync(h, acc, dacc.p, sizeof(acc), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, psum.data(), dpsum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (acc[64] > N || acc[65] > acc[64]) return fail(h, PPP_ERR_HIP, "contact field: statistics corrupt");
    st = {};
    st.n = N; st.valid = (size_t)acc[64]; st.narrow = (size_t)acc[65];
    st.min_abs_r = st.valid ? -ordered_unkey((unsigned)acc[66]) : NAN; st.max_abs_r = st.valid ? ordered_unkey((unsigned)acc[67]) : NAN;
    for (double v : psum) st.sum_abs_r += v;
    for (int b = 0; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[b];
    return PPP_OK;
}
static int field_statistics(ppp_handle h, float min_width)
{
    auto &C = h->field;
    int rc = field_statistics(h, C.hw.p, C.acc, C.psum, min_width, C.stats);
    if (!rc) C.min_width = min_width;
    return rc;
}

int ppp_get_contact_field(ppp_handle h, float *curv5, float *half_width, size_t cap, float min_width, ppp_contact_field_stats *stats)
{
    if (int rcb = whole_cloud_begin(h, "contact field", "the maps address the whole cloud")) return rcb;
    if (h->P.slice_begin != 0 || h->P.slice_end != 0)
        return fail(h, PPP_ERR_UNSUPPORTED, "contact field: a slice-range handle indexes a part of the cloud only");
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    if (!(min_width > 0.f)) min_width = 0.f;
    const size_t N = h->n;
    auto &C = h->field;
    const ppp_params &P = h->P, &F = C.P;
    const bool same = C.valid && same_contact_params(P, F);
    if (!same) {
        C.valid = false;
        int rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        if (h->ranged || h->use_part) return fail(h, PPP_ERR_UNSUPPORTED, "contact field: a slice-range handle indexes a part of the cloud only");
        rc = contact_buffers(h);
        if (rc) return rc;
        const size_t N1 = std::max<size_t>(N, 1);
        HIPCHK(h, C.curv.ensure(5 * N1)); HIPCHK(h, C.hw.ensure(N1));
        HIPCHK(h, hipMemsetAsync(C.curv.p, 0xff, 5 * N1 * sizeof(float), h->stream)); /* dropped points: NaN */
        HIPCHK(h, hipMemsetAsync(C.hw.p, 0xff, N1 * sizeof(float), h->stream));
        const int nsorted = h->hmeta.n_sorted;
        if (nsorted < 0 || (size_t)nsorted > N) return fail(h, PPP_ERR_HIP, "contact field: index corrupt");
        if (nsorted > 0) /* a wave per FIELD_Q indexed points, in slab / y order */
            LAUNCH(h, "k_field_batch", k_field_batch, (unsigned)((nsorted + FIELD_Q * DYN_WAVES - 1) / (FIELD_Q * DYN_WAVES)), 64 * DYN_WAVES, 0,
                   contact_index(h), dyn_params(h), nsorted, C.curv.p, C.hw.p);
        rc = field_statistics(h, min_width);
        if (rc) return rc;
        C.P = h->P;
        C.valid = true; ++C.built;
    } else if (stats && min_width != C.min_width) {
        int rc = field_statistics(h, min_width);
        if (rc) return rc;
    }
    if (stats) *stats = C.stats;
    const size_t k = std::min(cap, N);
    if (curv5 && k) HIPCHK(h, copy_sync(h, curv5, C.curv.p, 5 * k * sizeof(float), hipMemcpyDeviceToHost));
    if (half_width && k) HIPCHK(h, copy_sync(h, half_width, C.hw.p, k * sizeof(float), hipMemcpyDeviceToHost));
    return PPP_OK;
}

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
static int deviation_call_ok(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp, const std::string &w, const float *halo)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!ref || !dp) return fail(h, PPP_ERR_ARG, w + ": no reference handle or no parameters");
    const ppp_deviation_params &P = *dp;
    if (!(P.max_dist > 0.f)) return fail(h, PPP_ERR_ARG, w + (halo ? ": max_dist must be > 0" : ": max_dist must be > 0 (+INFINITY: no limit)"));
    if (halo && !std::isfinite(P.max_dist)) return fail(h, PPP_ERR_ARG, w + ": a tile needs a finite max_dist: the halo must hold every partner");
    if (!(P.smooth_radius >= 0.f && std::isfinite(P.smooth_radius))) return fail(h, PPP_ERR_ARG, w + ": smooth_radius must be finite and >= 0");
    if (!std::isfinite(P.allowance)) return fail(h, PPP_ERR_ARG, w + ": allowance must be finite");
    if (!(P.gain >= 0.0 && std::isfinite(P.gain))) return fail(h, PPP_ERR_ARG, w + ": gain must be finite and >= 0");
    if (!halo && P.smooth_radius > 0.f && !std::isfinite(P.max_dist)) return fail(h, PPP_ERR_ARG, w + ": smoothing needs a finite max_dist");
    if (halo && !(*halo >= P.max_dist + P.smooth_radius && *halo <= 3.402823466e+38f))
        return fail(h, PPP_ERR_ARG, w + ": halo must be finite and at least max_dist + smooth_radius");
    if (ref->device != h->device) return fail(h, PPP_ERR_ARG, w + ": the two handles are on different devices");
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
    const int grid = parts.grid, per = parts.per, nq = h->hmeta.n_sorted, nref = ref->hmeta.n_sorted;
    HIPCHK(h, D.dev.ensure(N1)); HIPCHK(h, D.target.ensure(N1)); HIPCHK(h, D.fix.ensure(N1)); HIPCHK(h, D.d2.ensure(N1));
    HIPCHK(h, D.ref_index.ensure(N1)); HIPCHK(h, D.status.ensure(N1)); HIPCHK(h, D.acc.ensure(DEV_ACC_WORDS)); HIPCHK(h, D.psum.ensure(2 * (size_t)grid));
    if (smooth) HIPCHK(h, D.smoothed.ensure(N1));
    double *v = smooth ? D.smoothed.p : D.dev.p;
    HIPCHK(h, hipMemsetAsync(D.status.p, PPP_DEV_DROPPED, N1, h->stream)); /* points outside the index: not finite */
    HIPCHK(h, hipMemsetAsync(D.ref_index.p, 0xff, N1 * sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(D.acc.p, 0, DEV_ACC_WORDS * sizeof(unsigned long long), h->stream));
    const unsigned gq = (unsigned)((nq + DEV_T - 1) / DEV_T);
    if (nq > 0) {
        LAUNCH(h, "k_dev_nearest", k_dev_nearest, gq, DEV_T, 0, h->sorted4.p, nq, contact_index(ref), nref, P.max_dist * P.max_dist, D.dev.p, D.fix.p,
               D.d2.p, D.ref_index.p, D.status.p);
        if (smooth)
            LAUNCH(h, "k_dev_smooth", k_dev_smooth, gq, DEV_T, 0, contact_index(h), nq, P.smooth_radius * P.smooth_radius, D.status.p, D.fix.p,
                   D.smoothed.p);
    }
    LAUNCH(h, "k_dev_target", k_dev_target, (unsigned)std::min<size_t>((N1 + DEV_T - 1) / DEV_T, 2 * (size_t)h->num_cus), DEV_T, 0, D.status.p,
           D.dev.p, v, D.d2.p, (int)N, P.allowance, P.gain, D.target.p, D.acc.p);
    LAUNCH(h, "k_dev_stats", k_dev_stats, (unsigned)grid, PCON_T, 0, D.status.p, v, D.target.p, (int)N, per, D.acc.p, D.psum.p, D.psum.p + grid);
    unsigned long long acc[DEV_ACC_WORDS];
    std::vector<double> psum(2 * (size_t)grid);
    HIPCHK(h, copy_sync(h, acc, D.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
    HIPCHK(h, copy_sync(h, psum.data(), D.psum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (acc[0] + acc[1] + acc[2] + acc[3] != N || acc[DEV_ACC_PROUD] > acc[0] || acc[DEV_ACC_BELOW] > acc[0])
        return fail(h, PPP_ERR_HIP, "deviation: statistics corrupt");
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
    double ext[3];
    for (int d = 0; d < 3; ++d) {
        F.c[d] = ((double)ref->hmeta.mn[d] + (double)ref->hmeta.mx[d]) * 0.5;
        ext[d] = (double)ref->hmeta.mx[d] - (double)ref->hmeta.mn[d];
    }
    F.Ln = (((ext[0] + ext[1]) + ext[2]) * 0.5) + (double)P.max_dist;
    F.scale = std::ldexp(1.0, shift);
    return reference_normals(h, ref, "registration");
}

/* a chain's control words behind the one wait: 0 <= steps <= iterations, and a chain that has not ended took every step */
static bool chain_ctl_ok(const IcpCtl &c, int iterations) { return c.steps >= 0 && c.steps <= iterations && (c.done || c.steps == iterations); }

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
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (T0) memcpy(T, T0, sizeof(T));
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) return fail(h, PPP_ERR_ARG, "registration: the transform has an entry that is not finite");
    int shift = 0;
    rc = registration_setup(h, ref, P, F, shift);
    if (rc) return rc;
    const size_t N = h->n;
    const int nq = h->hmeta.n_sorted, nref = ref->hmeta.n_sorted;
    static_assert(sizeof(IcpCtl) == 5 * sizeof(int), "IcpCtl is five ints");
    auto &G = h->registration;
    const size_t evals = (size_t)iterations + 1;
    HIPCHK(h, G.T.ensure(12 * evals)); HIPCHK(h, G.acc.ensure(ICP_WORDS * evals)); HIPCHK(h, G.rows.ensure(evals)); HIPCHK(h, G.ctl.ensure(8));
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.ctl.p);
    HIPCHK(h, hipMemsetAsync(G.acc.p, 0, ICP_WORDS * evals * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(G.ctl.p, 0, 8 * sizeof(int), h->stream));
    HIPCHK(h, copy_sync(h, G.T.p, T, sizeof(T), hipMemcpyHostToDevice));
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
    HIPCHK(h, copy_sync(h, &C, G.ctl.p, sizeof(C), hipMemcpyDeviceToHost)); /* the one wait */
    if (!chain_ctl_ok(C, iterations)) return fail(h, PPP_ERR_HIP, "registration: control words corrupt");
    const size_t last = (size_t)C.steps;
    std::vector<ppp_registration_row> R(last + 1);
    HIPCHK(h, copy_sync(h, R.data(), G.rows.p, (last + 1) * sizeof(ppp_registration_row), hipMemcpyDeviceToHost));
    if (!C.done) { /* the evaluation behind the last step: no step kernel follows it */
        unsigned long long acc[ICP_WORDS];
        double Tl[12];
        HIPCHK(h, copy_sync(h, acc, G.acc.p + ICP_WORDS * last, sizeof(acc), hipMemcpyDeviceToHost));
        HIPCHK(h, copy_sync(h, Tl, G.T.p + 12 * last, sizeof(Tl), hipMemcpyDeviceToHost));
        icp_row_terms(&R[last], Tl, acc);
    }
    if (R[0].pairs > (size_t)std::max(nq, 0) || R[last].pairs > (size_t)std::max(nq, 0)) return fail(h, PPP_ERR_HIP, "registration: sums corrupt");
    if (stats) {
        ppp_registration_stats st = {};
        st.n = N; st.indexed = (size_t)nq;
        st.steps = C.steps; st.converged = C.converged; st.locked = C.locked; st.shift = shift;
        for (int d = 0; d < 3; ++d) st.centre[d] = F.c[d];
        st.length = F.Ln;
        memcpy(st.T, R[last].T, sizeof(st.T));
        auto rms = [&](const ppp_registration_row &r) {
            return r.pairs ? std::sqrt(std::ldexp((double)r.E, -shift) / (double)r.pairs) : (double)NAN;
        };
        st.pairs_before = R[0].pairs; st.rms_before = rms(R[0]);
        st.pairs_after = R[last].pairs; st.rms_after = rms(R[last]);
        *stats = st;
    }
    const size_t k = std::min(row_cap, last + 1);
    if (rows && k) memcpy(rows, R.data(), k * sizeof(ppp_registration_row));
    if (trim) {
        std::vector<TrimCut> cut(last + 1);
        HIPCHK(h, copy_sync(h, cut.data(), G.cuts.p, (last + 1) * sizeof(TrimCut), hipMemcpyDeviceToHost));
        for (size_t i = 0; i <= last; ++i)
            if (cut[i].paired > (unsigned)std::max(nq, 0) || R[i].pairs > cut[i].paired || (cut[i].paired && R[i].pairs < cut[i].k))
                return fail(h, PPP_ERR_HIP, "trimmed registration: cut corrupt");
        for (size_t i = 0; trim->rows && i < k; ++i) {
            ppp_trimmed_registration_row &o = trim->rows[i];
            memset(&o, 0, sizeof(o)); /* the padding too: rows compare as bytes */
            o.row = R[i];
            o.paired = cut[i].paired;
            memcpy(&o.trim_d2, &cut[i].tau, sizeof(float));
        }
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
        double ext[3];
        for (int d = 0; d < 3; ++d) {
            F.c[d] = ((double)side->hmeta.mn[d] + (double)side->hmeta.mx[d]) * 0.5;
            ext[d] = (double)side->hmeta.mx[d] - (double)side->hmeta.mn[d];
        }
        F.L = ((ext[0] + ext[1]) + ext[2]) * 0.5;
        if (!(F.L > 0.0 && std::isfinite(F.L))) return fail(side, PPP_ERR_ARG, "the box of the cloud has no extent (L == 0)");
        const int ms = mom_shift(side->n);
        F.scale = std::ldexp(1.0, ms);
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

/* Global registration: both clouds' moments, the starts their frames imply, then every start's coarse chain
   side by side -- coarse.iterations + 1 launches of k_reg_terms_multi and coarse.iterations of k_reg_step_multi back to back
   on h's stream, on the queries compacted once -- one wait, the winner by cost on the host, and registration_chain from it. */
int ppp_register_global(ppp_handle h, ppp_handle ref, const ppp_global_registration_params *gp, ppp_registration_candidate *cands, size_t cand_cap,
                        ppp_registration_row *rows, size_t row_cap, ppp_global_registration_stats *stats)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!ref || !gp) return fail(h, PPP_ERR_ARG, "global registration: no reference handle or no parameters");
    if (!rows && row_cap) return fail(h, PPP_ERR_ARG, "global registration: rows is NULL with row_cap > 0");
    if (!cands && cand_cap) return fail(h, PPP_ERR_ARG, "global registration: cands is NULL with cand_cap > 0");
    const ppp_global_registration_params P = *gp;
    if (P.candidates != 4 && P.candidates != 24) return fail(h, PPP_ERR_ARG, "global registration: candidates must be 4 or 24");
    if (P.stride < 1) return fail(h, PPP_ERR_ARG, "global registration: stride must be >= 1");
    IcpFrame F, Ffine;
    int rc = registration_params_ok(h, P.coarse, F);
    if (rc) return rc;
    rc = registration_params_ok(h, P.fine, Ffine);
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
    const int K = P.candidates, iterations = P.coarse.iterations;
    const size_t evals = (size_t)iterations + 1;
    std::vector<double> T((size_t)K * evals * 12, 0.0), T0((size_t)K * 12);
    registration_starts(&st.scan, &st.ref, K, T0.data());
    for (double v : T0) if (!std::isfinite(v)) return fail(h, PPP_ERR_ARG, "global registration: a start has an entry that is not finite");
    for (int s = 0; s < K; ++s) memcpy(&T[(size_t)s * evals * 12], &T0[(size_t)s * 12], 12 * sizeof(double));
    const int ns = h->hmeta.n_sorted, nref = ref->hmeta.n_sorted;
    auto &G = h->registration;
    static_assert(sizeof(IcpCtl) == 5 * sizeof(int), "IcpCtl is five ints");
    const size_t ns1 = (size_t)std::max(ns, 1);
    HIPCHK(h, G.queries.ensure(ns1)); HIPCHK(h, G.qcnt.ensure((ns1 + COMPACT_CHUNK - 1) / COMPACT_CHUNK + 1));
    HIPCHK(h, G.mT.ensure(T.size())); HIPCHK(h, G.macc.ensure(ICP_WORDS * evals * K)); HIPCHK(h, G.mrows.ensure(evals * K)); HIPCHK(h, G.mctl.ensure(5 * (size_t)K));
    int nq = 0;
    if (ns > 0) {
        const int nblocks = (ns + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
        StrideSel sel = {h->sorted4.p, P.stride, G.queries.p};
        rc = compact(h, sel, ns, G.qcnt.p, G.qcnt.p + nblocks, [&](int kept) -> int {
            if (kept < 0 || kept > ns) return fail(h, PPP_ERR_HIP, "global registration: query count corrupt");
            nq = kept;
            return PPP_OK;
        });
        if (rc) return rc;
    }
    if (nq <= 0) return fail(h, PPP_ERR_ARG, "global registration: no query left (no indexed point has a cloud index that is a multiple of stride)");
    HIPCHK(h, hipMemsetAsync(G.macc.p, 0, ICP_WORDS * evals * K * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(G.mctl.p, 0, 5 * (size_t)K * sizeof(int), h->stream));
    HIPCHK(h, copy_sync(h, G.mT.p, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));
    IcpCtl *ctl = reinterpret_cast<IcpCtl *>(G.mctl.p);
    /* all starts together stay at two workgroups per CU, and never below one per start */
    const size_t per = std::max<size_t>(1, std::min<size_t>(((size_t)nq + ICP_T - 1) / ICP_T, 2 * (size_t)h->num_cus / (size_t)K));
    const size_t tstride = 12 * evals, astride = ICP_WORDS * evals;
    for (int k = 0; k <= iterations; ++k) {
        LAUNCH(h, "k_reg_terms_multi", k_reg_terms_multi, dim3((unsigned)per, (unsigned)K), ICP_T, 0, G.queries.p, nq, contact_index(ref), nref, F,
               G.mT.p + 12 * (size_t)k, tstride, ctl, G.macc.p + ICP_WORDS * (size_t)k, astride);
        if (k < iterations)
            LAUNCH(h, "k_reg_step_multi", k_reg_step_multi, K, 64, 0, G.macc.p + ICP_WORDS * (size_t)k, astride, F, G.mT.p + 12 * (size_t)k, tstride,
                   G.mrows.p + k, evals, ctl);
    }
    std::vector<IcpCtl> C((size_t)K);
    std::vector<ppp_registration_row> R(evals * K);
    std::vector<unsigned long long> acc(ICP_WORDS * evals * K);
    HIPCHK(h, copy_sync(h, C.data(), G.mctl.p, C.size() * sizeof(IcpCtl), hipMemcpyDeviceToHost)); /* the one wait */
    HIPCHK(h, copy_sync(h, R.data(), G.mrows.p, R.size() * sizeof(ppp_registration_row), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, acc.data(), G.macc.p, acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, T.data(), G.mT.p, T.size() * sizeof(double), hipMemcpyDeviceToHost));
    const long long far = llrint((double)F.md2 * F.scale);
    std::vector<ppp_registration_candidate> cd((size_t)K);
    int win = 0;
    for (int s = 0; s < K; ++s) {
        const IcpCtl &c = C[(size_t)s];
        if (!chain_ctl_ok(c, iterations)) return fail(h, PPP_ERR_HIP, "global registration: control words corrupt");
        const size_t first = (size_t)s * evals, last = first + (size_t)c.steps;
        if (!c.done) icp_row_terms(&R[last], &T[12 * last], &acc[ICP_WORDS * last]); /* the evaluation behind the last step: no step kernel follows it */
        if (R[first].pairs > (size_t)nq || R[last].pairs > (size_t)nq) return fail(h, PPP_ERR_HIP, "global registration: sums corrupt");
        ppp_registration_candidate &o = cd[(size_t)s];
        o = ppp_registration_candidate{};
        o.index = s;
        memcpy(o.T0, &T0[12 * (size_t)s], sizeof(o.T0)); memcpy(o.T, R[last].T, sizeof(o.T));
        o.steps = c.steps; o.converged = c.converged; o.locked = c.locked;
        o.pairs0 = R[first].pairs; o.E0 = R[first].E; o.pairs = R[last].pairs; o.E = R[last].E;
        o.cost = o.E + (long long)((size_t)nq - o.pairs) * far;
        if (o.cost < cd[(size_t)win].cost) win = s;
    }
    long long second = -1;
    for (int s = 0; s < K; ++s)
        if (memcmp(cd[(size_t)s].T, cd[(size_t)win].T, sizeof(cd[0].T)) != 0 && (second < 0 || cd[(size_t)s].cost < second)) second = cd[(size_t)s].cost;
    rc = registration_chain(h, ref, &P.fine, cd[(size_t)win].T, true, rows, row_cap, &st.fine);
    if (rc) return rc;
    st.queries = (size_t)nq; st.shift = shift; st.candidates = K; st.winner = win;
    st.winner_cost = cd[(size_t)win].cost; st.second_cost = second;
    if (stats) *stats = st;
    const size_t k = std::min(cand_cap, (size_t)K);
    if (cands && k) memcpy(cands, cd.data(), k * sizeof(ppp_registration_candidate));
    return PPP_OK;
}

/* What this handle's tile evaluates and owns, behind a plan: the cuts of its range [sb, se) on the walk of the
   whole cloud's bounds, widened by halo; a whole-cloud handle owns and evaluates everything. */
static int tile_range(ppp_handle h, float halo, TileRange &T)
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
static bool leaves_indexed_range(const ppp_handle h, float lo, float hi)
{
    return h->ranged && lo <= hi && ((lo < h->incl_lo && h->incl_lo > h->h_mn[0]) || (hi > h->incl_hi && h->incl_hi < h->h_mx[0]));
}

/* the positions [pos0, pos1) of the slabs that meet the tile's evaluated interval (one slab more on either side: the kernels
   test every point themselves), behind index_ready */
static int tile_positions(ppp_handle h, const TileRange &T, int &pos0, int &pos1)
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

static void tile_field_stats(ppp_contact_field_tile_stats &o, const ppp_contact_field_stats &st)
{
    o.n = st.n; o.valid = st.valid; o.narrow = st.narrow; o.min_abs_r = st.min_abs_r; o.max_abs_r = st.max_abs_r; o.sum_abs_r = st.sum_abs_r;
    memcpy(o.hist, st.hist, sizeof(o.hist));
}

int ppp_get_contact_field_tile(ppp_handle h, float *curv5, float *half_width, unsigned char *owned, size_t cap, float halo,
                               float min_width, ppp_contact_field_tile_stats *stats)
{
    if (int rcb = whole_cloud_begin(h, "contact field tile", "the maps address the whole cloud")) return rcb;
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    if (!(halo >= 0.f && halo <= 3.402823466e+38f)) return fail(h, PPP_ERR_ARG, "contact field tile: halo must be a finite number >= 0");
    if (!(min_width > 0.f)) min_width = 0.f;
    const size_t N = h->n;
    auto &C = h->ftile;
    const ppp_params &P = h->P, &F = C.P;
    const bool same = C.valid && same_contact_params(P, F) && P.walk == F.walk && P.slice_begin == F.slice_begin && P.slice_end == F.slice_end &&
                      P.range_margin == F.range_margin && halo == C.halo;
    if (!same) {
        C.valid = false;
        int rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        rc = contact_buffers(h);
        if (rc) return rc;
        TileRange T;
        rc = tile_range(h, halo, T);
        if (rc) return rc;
        int pos0, pos1;
        rc = tile_positions(h, T, pos0, pos1);
        if (rc) return rc;
        const size_t N1 = std::max<size_t>(N, 1);
        HIPCHK(h, C.curv.ensure(5 * N1)); HIPCHK(h, C.hw.ensure(N1)); HIPCHK(h, C.hw_own.ensure(N1)); HIPCHK(h, C.owned.ensure(N1));
        HIPCHK(h, C.cnt.ensure(4));
        HIPCHK(h, hipMemsetAsync(C.curv.p, 0xff, 5 * N1 * sizeof(float), h->stream)); /* not evaluated: NaN */
        HIPCHK(h, hipMemsetAsync(C.hw.p, 0xff, N1 * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(C.hw_own.p, 0xff, N1 * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(C.owned.p, 0, N1, h->stream));
        HIPCHK(h, hipMemsetAsync(C.cnt.p, 0, 4 * sizeof(int), h->stream));
        if (pos1 > pos0) {
            const int np = pos1 - pos0;
            LAUNCH(h, "k_tile_mark", k_tile_mark, (unsigned)((np + PCON_T - 1) / PCON_T), PCON_T, 0, h->sorted4.p, pos0, pos1, T, C.owned.p, C.cnt.p);
            LAUNCH(h, "k_field_tile", k_field_tile, (unsigned)((np + FIELD_Q * DYN_WAVES - 1) / (FIELD_Q * DYN_WAVES)), 64 * DYN_WAVES, 0,
                   contact_index(h), dyn_params(h), pos0, pos1, T, pcov_range(h), C.curv.p, C.hw.p, C.hw_own.p, C.cnt.p + 2);
        }
        int cnt[3];
        HIPCHK(h, copy_sync(h, cnt, C.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
        if (cnt[2])
            return fail(h, PPP_ERR_CAPACITY, "contact field tile: a search of an evaluated point (its neighbours or their normals) reaches beyond the indexed slice range: raise range_margin");
        if (cnt[0] < 0 || cnt[1] < cnt[0] || (size_t)cnt[1] > N) return fail(h, PPP_ERR_HIP, "contact field tile: counts corrupt");
        ppp_contact_field_stats st;
        rc = field_statistics(h, C.hw_own.p, C.acc, C.psum, min_width, st);
        if (rc) return rc;
        C.stats = {};
        C.stats.owned = (size_t)cnt[0]; C.stats.evaluated = (size_t)cnt[1]; C.stats.own_lo = T.own_lo; C.stats.own_hi = T.own_hi;
        tile_field_stats(C.stats, st);
        C.P = h->P; C.halo = halo; C.min_width = min_width;
        C.valid = true; ++C.built;
    } else if (stats && min_width != C.min_width) {
        ppp_contact_field_stats st;
        int rc = field_statistics(h, C.hw_own.p, C.acc, C.psum, min_width, st);
        if (rc) return rc;
        tile_field_stats(C.stats, st);
        C.min_width = min_width;
    }
    if (stats) *stats = C.stats;
    const size_t k = std::min(cap, N);
    if (curv5 && k) HIPCHK(h, copy_sync(h, curv5, C.curv.p, 5 * k * sizeof(float), hipMemcpyDeviceToHost));
    if (half_width && k) HIPCHK(h, copy_sync(h, half_width, C.hw.p, k * sizeof(float), hipMemcpyDeviceToHost));
    if (owned && k) HIPCHK(h, copy_sync(h, owned, C.owned.p, k, hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* lanes per selected point in k_reg_link */
#ifndef REG_GROUP
#define REG_GROUP 8
#endif

/* The device work of a region call, behind index_ready and the source's own call: select inside T's evaluated interval, list,
   link, flatten (T's owned points count), label, the rows in ascending label -- into h->regions' buffers.  half_width: the map
   PPP_REGIONS_NARROW reads.  nsel / nreg: the listed points and the regions (a tile's: every component of the list). */
static int regions_compute(ppp_handle h, int source, const unsigned char *mask, const float *half_width, float threshold, float link,
                           const TileRange &T, size_t &nsel, size_t &nreg, unsigned tot[4])
{
    const size_t N = h->n;
    auto &R = h->regions;
    R.valid = false;
    nsel = nreg = 0;
    const int ns = h->hmeta.n_sorted;
    if (ns < 0 || (size_t)ns > N || N > 0x7fffffffu) return fail(h, PPP_ERR_HIP, "regions: index corrupt");
    const size_t N1 = std::max<size_t>(N, 1);
    const int nb_sel = (ns + COMPACT_CHUNK - 1) / COMPACT_CHUNK, nb_head = (int)((N + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
    HIPCHK(h, R.labels.ensure(N1)); HIPCHK(h, R.head_root.ensure(N1)); HIPCHK(h, R.tot.ensure(8));
    HIPCHK(h, R.cnt.ensure((size_t)std::max(nb_sel, nb_head) + 1));
    HIPCHK(h, hipMemsetAsync(R.labels.p, 0xff, N1 * sizeof(int), h->stream)); /* not selected: -1 */
    HIPCHK(h, hipMemsetAsync(R.tot.p, 0, 8 * sizeof(unsigned), h->stream));
    int *err = (int *)R.tot.p + 3;
    int rc = PPP_OK;
    if (ns > 0) {
        HIPCHK(h, R.sel.ensure((size_t)ns)); HIPCHK(h, R.ord.ensure((size_t)ns));
        HIPCHK(h, hipMemsetAsync(R.ord.p, 0xff, (size_t)ns * sizeof(int), h->stream));
        RegSource S = {source, nullptr, nullptr, nullptr, nullptr, threshold};
        if (source == PPP_REGIONS_UNCOVERED) S.bytes = h->pcov.flags.p;
        else if (source == PPP_REGIONS_OVERLAP) { S.first = h->pcon.first.p; S.last = h->pcon.last.p; }
        else if (source == PPP_REGIONS_NARROW) S.half_width = half_width;
        else {
            HIPCHK(h, R.mask.ensure(N1));
            HIPCHK(h, hipMemcpyAsync(R.mask.p, mask, N, hipMemcpyHostToDevice, h->stream));
            S.bytes = R.mask.p;
        }
        LAUNCH(h, "k_reg_select", k_reg_select, (unsigned)((ns + REG_T - 1) / REG_T), REG_T, 0, h->sorted4.p, ns, S, T, R.sel.p);
        RegSel sel = {R.sel.p, nullptr, R.ord.p, nullptr, nullptr};
        rc = compact(h, sel, ns, R.cnt.p, (int *)R.tot.p + 4, [&](int kept) -> int {
            if (kept < 0 || kept > ns) return fail(h, PPP_ERR_HIP, "regions: selection count corrupt");
            nsel = (size_t)kept;
            HIPCHK(h, R.list.ensure(nsel)); HIPCHK(h, R.parent.ensure(nsel)); HIPCHK(h, R.acc.ensure(nsel));
            sel.list = R.list.p; sel.parent = R.parent.p; sel.acc = R.acc.p;
            return PPP_OK;
        });
        if (rc) return rc;
    }
    if (nsel > 0) {
        const float r2 = link * link;
        int grp = REG_GROUP;
        if (const char *ev = tuning_env("PPP_REG_GROUP")) grp = atoi(ev); /* tuning runs only */
        const unsigned gl = (unsigned)((nsel * (size_t)grp + REG_T - 1) / REG_T), gp = (unsigned)((nsel + REG_T - 1) / REG_T);
#define PPP_REG_LINK(G) LAUNCH(h, "k_reg_link", k_reg_link<G>, gl, REG_T, 0, h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_ytab.p, R.list.p, (int)nsel, R.ord.p, R.parent.p, link, r2, err)
        if (grp == 1) PPP_REG_LINK(1);
        else if (grp == 4) PPP_REG_LINK(4);
        else if (grp == 16) PPP_REG_LINK(16);
        else if (grp == 64) PPP_REG_LINK(64);
        else if (grp == 8) PPP_REG_LINK(8);
        else return fail(h, PPP_ERR_ARG, "regions: PPP_REG_GROUP must be 1, 4, 8, 16 or 64");
#undef PPP_REG_LINK
        LAUNCH(h, "k_reg_flatten", k_reg_flatten, gp, REG_T, 0, h->sorted4.p, R.list.p, (int)nsel, R.parent.p, R.acc.p, T, err);
        LAUNCH(h, "k_reg_labels", k_reg_labels, gp, REG_T, 0, h->sorted4.p, R.list.p, (int)nsel, R.parent.p, R.acc.p, (int)N, R.labels.p,
               R.head_root.p, R.tot.p);
        RegHeadSel heads = {R.labels.p, R.head_root.p, R.acc.p, nullptr};
        rc = compact(h, heads, (int)N, R.cnt.p, (int *)R.tot.p + 5, [&](int kept) -> int {
            if (kept < 0 || (size_t)kept > nsel) return fail(h, PPP_ERR_HIP, "regions: region count corrupt");
            nreg = (size_t)kept;
            HIPCHK(h, R.rows.ensure(nreg));
            heads.rows = R.rows.p;
            return PPP_OK;
        });
        if (rc) return rc;
    }
    HIPCHK(h, copy_sync(h, tot, R.tot.p, 4 * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (tot[3]) return fail(h, PPP_ERR_CAPACITY, "regions: a union-find walk reached its trip cap");
    if (tot[0] != nreg || tot[1] > nreg || tot[2] > nsel) return fail(h, PPP_ERR_HIP, "regions: totals corrupt");
    return PPP_OK;
}

/* the opening of every region call (whole_cloud_begin) and its argument checks */
static int regions_begin(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius)
{
    if (int rcb = whole_cloud_begin(h, "regions", "a region does not stop at a part's border")) return rcb;
    if (source < PPP_REGIONS_UNCOVERED || source > PPP_REGIONS_MASK) return fail(h, PPP_ERR_ARG, "regions: unknown source");
    if (source == PPP_REGIONS_MASK && !mask) return fail(h, PPP_ERR_ARG, "regions: PPP_REGIONS_MASK needs a mask");
    if (source == PPP_REGIONS_NARROW && !(threshold > 0.f && threshold <= 3.402823466e+38f))
        return fail(h, PPP_ERR_ARG, "regions: PPP_REGIONS_NARROW needs a positive finite threshold");
    if (!(fabsf(link_radius) <= 3.402823466e+38f)) return fail(h, PPP_ERR_ARG, "regions: link_radius is not a finite number");
    return PPP_OK;
}

/* could a region's fixed-point sum leave 64 bits?  then no centroid is given (B.34) */
static bool regions_nan_centroid(double reach, size_t selected) { return reach * REG_FIXED * (double)selected >= 4611686018427387904.0; }

int ppp_get_regions(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius, int *labels, size_t cap,
                    ppp_region *regions, size_t region_cap, ppp_region_stats *stats)
{
    { int rca = regions_begin(h, source, mask, threshold, link_radius); if (rca) return rca; }
    if (h->P.slice_begin != 0 || h->P.slice_end != 0)
        return fail(h, PPP_ERR_UNSUPPORTED, "regions: a region does not stop at a range border: a slice-range handle indexes a part of the cloud only");
    const float link = link_radius > 0.f ? link_radius : h->P.normal_radius;
    if (source != PPP_REGIONS_NARROW) threshold = 0.f;
    /* the source's own call: builds its result if the handle does not hold it, answers from it if it does, refuses as it does */
    unsigned long long serial = 0;
    int rc = PPP_OK;
    if (source == PPP_REGIONS_UNCOVERED) { rc = ppp_get_path_coverage(h, nullptr, 0, nullptr, nullptr); serial = h->pcov.serial; }
    else if (source == PPP_REGIONS_OVERLAP) { rc = ppp_get_path_contacts(h, nullptr, nullptr, nullptr, 0, nullptr); serial = h->pcon.serial; }
    else if (source == PPP_REGIONS_NARROW) { rc = ppp_get_contact_field(h, nullptr, nullptr, 0, 0.f, nullptr); serial = h->field.built; }
    if (rc) return rc;
    const size_t N = h->n;
    auto &R = h->regions;
    const bool reuse = source != PPP_REGIONS_MASK && R.valid && R.source == source && R.threshold == threshold && R.link == link &&
                       R.serial == serial && R.stats.n == N;
    if (!reuse) {
        R.valid = false;
        rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        if (h->ranged || h->use_part) return fail(h, PPP_ERR_UNSUPPORTED, "regions: a slice-range handle indexes a part of the cloud only");
        double reach = 0.0; /* the largest |coordinate| of the index */
        for (int d = 0; d < 3; ++d) reach = std::max(reach, std::max(std::fabs((double)h->hmeta.mn[d]), std::fabs((double)h->hmeta.mx[d])));
        size_t nsel = 0, nreg = 0;
        unsigned tot[4];
        rc = regions_compute(h, source, mask, h->field.hw.p, threshold, link, TileRange{-INFINITY, INFINITY, -INFINITY, INFINITY}, nsel, nreg, tot);
        if (rc) return rc;
        ppp_region_stats st = {};
        st.n = N; st.selected = nsel; st.regions = nreg; st.singletons = tot[1]; st.largest = tot[2];
        R.stats = st;
        R.nan_centroid = regions_nan_centroid(reach, nsel);
        R.source = source; R.threshold = threshold; R.link = link; R.serial = serial;
        R.valid = true;
    }
    if (stats) *stats = R.stats;
    const size_t k = std::min(cap, N);
    if (labels && k) HIPCHK(h, copy_sync(h, labels, R.labels.p, k * sizeof(int), hipMemcpyDeviceToHost));
    const size_t kr = std::min(region_cap, R.stats.regions);
    if (regions && kr) {
        std::vector<RegAcc> rows(kr);
        HIPCHK(h, copy_sync(h, rows.data(), R.rows.p, kr * sizeof(RegAcc), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kr; ++i) {
            const RegAcc &a = rows[i];
            ppp_region &o = regions[i];
            o.label = a.label; o.count = a.count;
            for (int c = 0; c < 3; ++c) {
                o.mn[c] = -ordered_unkey(a.kmn[c]); o.mx[c] = ordered_unkey(a.kmx[c]);
                o.centroid[c] = R.nan_centroid ? (double)NAN : (double)a.sum[c] / (double)a.count / REG_FIXED;
            }
        }
    }
    return PPP_OK;
}

int ppp_get_regions_tile(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius, int *labels, size_t cap,
                         ppp_region_part *parts, size_t part_cap, ppp_region_halo *halos, size_t halo_cap, ppp_region_tile_stats *stats)
{
    int rc = regions_begin(h, source, mask, threshold, link_radius);
    if (rc) return rc;
    if (source == PPP_REGIONS_UNCOVERED || source == PPP_REGIONS_OVERLAP)
        return fail(h, PPP_ERR_UNSUPPORTED, "regions tile: a range's coverage knows its own slices' balls only: OR the ranges' flags (ppp_get_path_coverage) and pass the result as a mask (PPP_REGIONS_MASK)");
    const float link = link_radius > 0.f ? link_radius : h->P.normal_radius;
    if (source != PPP_REGIONS_NARROW) threshold = 0.f;
    unsigned long long serial = 0;
    if (source == PPP_REGIONS_NARROW) { /* the field of the owned points and a halo of one link radius */
        rc = ppp_get_contact_field_tile(h, nullptr, nullptr, nullptr, 0, link, 0.f, nullptr);
        if (rc) return rc;
        serial = h->ftile.built;
    }
    const size_t N = h->n;
    auto &Q = h->rtile;
    const bool reuse = source != PPP_REGIONS_MASK && Q.valid && Q.source == source && Q.threshold == threshold && Q.link == link &&
                       Q.serial == serial && Q.stats.n == N;
    if (!reuse) {
        Q.valid = false;
        rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        TileRange T;
        rc = tile_range(h, link, T);
        if (rc) return rc;
        if (leaves_indexed_range(h, T.ev_lo, T.ev_hi))
            return fail(h, PPP_ERR_CAPACITY, "regions tile: the owned interval widened by the link radius reaches beyond the indexed slice range: raise range_margin");
        const unsigned char *owned_map = h->ftile.owned.p;
        if (source == PPP_REGIONS_MASK) { /* the owned map of this range and link */
            int pos0, pos1;
            rc = tile_positions(h, T, pos0, pos1);
            if (rc) return rc;
            const size_t N1 = std::max<size_t>(N, 1);
            HIPCHK(h, Q.owned.ensure(N1)); HIPCHK(h, Q.cnt.ensure(2));
            HIPCHK(h, hipMemsetAsync(Q.owned.p, 0, N1, h->stream));
            HIPCHK(h, hipMemsetAsync(Q.cnt.p, 0, 2 * sizeof(int), h->stream));
            if (pos1 > pos0)
                LAUNCH(h, "k_tile_mark", k_tile_mark, (unsigned)((pos1 - pos0 + PCON_T - 1) / PCON_T), PCON_T, 0, h->sorted4.p, pos0, pos1, T,
                       Q.owned.p, Q.cnt.p);
            owned_map = Q.owned.p;
        }
        size_t nsel = 0, nreg = 0;
        unsigned tot[4];
        rc = regions_compute(h, source, mask, h->ftile.hw.p, threshold, link, T, nsel, nreg, tot);
        if (rc) return rc;
        /* the tile's view of the device result: labels of the owned points, the components with an owned point, their halo points */
        std::vector<unsigned char> own(N);
        std::vector<RegAcc> rows(nreg);
        Q.labels.assign(N, -1);
        if (N) HIPCHK(h, copy_sync(h, own.data(), owned_map, N, hipMemcpyDeviceToHost));
        if (N && nsel) HIPCHK(h, copy_sync(h, Q.labels.data(), h->regions.labels.p, N * sizeof(int), hipMemcpyDeviceToHost));
        if (nreg) HIPCHK(h, copy_sync(h, rows.data(), h->regions.rows.p, nreg * sizeof(RegAcc), hipMemcpyDeviceToHost));
        Q.parts.clear(); Q.halos.clear();
        size_t selected = 0;
        for (const RegAcc &a : rows) {
            if (!a.count) continue; /* a component of halo points alone: its owners' tiles report it */
            ppp_region_part o;
            o.label = a.label; o.count = a.count;
            for (int c = 0; c < 3; ++c) { o.mn[c] = -ordered_unkey(a.kmn[c]); o.mx[c] = ordered_unkey(a.kmx[c]); o.fsum[c] = a.sum[c]; }
            Q.parts.push_back(o);
            selected += a.count;
        }
        auto has_part = [&](int label) {
            auto it = std::lower_bound(Q.parts.begin(), Q.parts.end(), label, [](const ppp_region_part &r, int l) { return r.label < l; });
            return it != Q.parts.end() && it->label == label;
        };
        for (size_t i = 0; i < N; ++i) {
            if (own[i] == 1 || Q.labels[i] < 0) continue;
            if (own[i] == 2 && has_part(Q.labels[i])) Q.halos.push_back(ppp_region_halo{(int)i, Q.labels[i]});
            Q.labels[i] = -1;
        }
        ppp_region_tile_stats st = {};
        st.n = N; st.selected = selected; st.parts = Q.parts.size(); st.halo_points = Q.halos.size();
        for (int d = 0; d < 3; ++d) /* the whole cloud's bounds: the same on every handle of the cloud */
            st.max_abs_coord = std::max(st.max_abs_coord, std::max(std::fabs((double)h->h_mn[d]), std::fabs((double)h->h_mx[d])));
        st.own_lo = T.own_lo; st.own_hi = T.own_hi;
        Q.stats = st;
        Q.source = source; Q.threshold = threshold; Q.link = link; Q.serial = serial;
        Q.valid = true;
    }
    if (stats) *stats = Q.stats;
    const size_t k = std::min(cap, N), kp = std::min(part_cap, Q.parts.size()), kh = std::min(halo_cap, Q.halos.size());
    if (labels && k) memcpy(labels, Q.labels.data(), k * sizeof(int));
    if (parts && kp) memcpy(parts, Q.parts.data(), kp * sizeof(ppp_region_part));
    if (halos && kh) memcpy(halos, Q.halos.data(), kh * sizeof(ppp_region_halo));
    return PPP_OK;
}

int ppp_merge_region_tiles(size_t tiles, const int *const *labels, const ppp_region_part *const *parts, const ppp_region_halo *const *halos,
                           const ppp_region_tile_stats *stats, int *out_labels, size_t cap, ppp_region *regions, size_t region_cap,
                           ppp_region_stats *out_stats)
{
    if (!tiles || !labels || !parts || !halos || !stats) return PPP_ERR_ARG;
    const size_t N = stats[0].n;
    std::vector<size_t> first(tiles + 1, 0); /* node of (t, part j) = first[t] + j */
    size_t selected = 0;
    double reach = 0.0;
    for (size_t t = 0; t < tiles; ++t) {
        if (stats[t].n != N || !labels[t] || (stats[t].parts && !parts[t]) || (stats[t].halo_points && !halos[t])) return PPP_ERR_ARG;
        for (size_t j = 1; j < stats[t].parts; ++j) if (!(parts[t][j - 1].label < parts[t][j].label)) return PPP_ERR_ARG;
        first[t + 1] = first[t] + stats[t].parts;
        selected += stats[t].selected;
        reach = std::max(reach, stats[t].max_abs_coord);
    }
    auto node_of = [&](size_t t, int label) -> long long { /* -1: tile t has no part of that label */
        const ppp_region_part *b = parts[t], *e = b + stats[t].parts;
        const ppp_region_part *it = std::lower_bound(b, e, label, [](const ppp_region_part &r, int l) { return r.label < l; });
        return it != e && it->label == label ? (long long)(first[t] + (size_t)(it - b)) : -1;
    };
    /* who owns a point: the one tile that labels it */
    std::vector<int> owner(N, -1);
    for (size_t t = 0; t < tiles; ++t)
        for (size_t i = 0; i < N; ++i)
            if (labels[t][i] >= 0) {
                if (owner[i] >= 0) return PPP_ERR_ARG; /* owned twice */
                owner[i] = (int)t;
            }
    const size_t nodes = first[tiles];
    std::vector<size_t> parent(nodes);
    for (size_t v = 0; v < nodes; ++v) parent[v] = v;
    auto find = [&](size_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
    for (size_t t = 0; t < tiles; ++t)
        for (size_t e = 0; e < stats[t].halo_points; ++e) {
            const ppp_region_halo &hp = halos[t][e];
            if (hp.cloud_index < 0 || (size_t)hp.cloud_index >= N || owner[(size_t)hp.cloud_index] < 0) return PPP_ERR_ARG; /* nobody's point */
            const size_t u = (size_t)owner[(size_t)hp.cloud_index];
            const long long a = node_of(t, hp.label), b = node_of(u, labels[u][(size_t)hp.cloud_index]);
            if (a < 0 || b < 0) return PPP_ERR_ARG;
            const size_t ra = find((size_t)a), rb = find((size_t)b);
            if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
        }
    /* the merged rows: integer sums, minima and maxima (as ordered keys: the order the device's atomics fold in) */
    struct Row { int label; unsigned long long count; unsigned kmn[3], kmx[3]; long long sum[3]; };
    std::vector<Row> acc(nodes, Row{0x7fffffff, 0, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}});
    for (size_t t = 0; t < tiles; ++t)
        for (size_t j = 0; j < stats[t].parts; ++j) {
            const ppp_region_part &p = parts[t][j];
            Row &r = acc[find(first[t] + j)];
            r.label = std::min(r.label, p.label); r.count += p.count;
            for (int c = 0; c < 3; ++c) {
                r.kmn[c] = std::max(r.kmn[c], ordered_key(-p.mn[c])); r.kmx[c] = std::max(r.kmx[c], ordered_key(p.mx[c]));
                r.sum[c] = (long long)((unsigned long long)r.sum[c] + (unsigned long long)p.fsum[c]);
            }
        }
    std::vector<size_t> roots;
    for (size_t v = 0; v < nodes; ++v) if (parent[v] == v) roots.push_back(v);
    std::sort(roots.begin(), roots.end(), [&](size_t a, size_t b) { return acc[a].label < acc[b].label; });
    ppp_region_stats st = {};
    st.n = N; st.selected = selected; st.regions = roots.size();
    for (size_t v : roots) { st.singletons += acc[v].count == 1; st.largest = std::max(st.largest, (size_t)acc[v].count); }
    if (out_stats) *out_stats = st;
    const bool nan_centroid = regions_nan_centroid(reach, selected);
    const size_t kr = std::min(region_cap, roots.size());
    for (size_t i = 0; regions && i < kr; ++i) {
        const Row &a = acc[roots[i]];
        ppp_region &o = regions[i];
        o.label = a.label; o.count = (unsigned)a.count;
        for (int c = 0; c < 3; ++c) {
            o.mn[c] = -ordered_unkey(a.kmn[c]); o.mx[c] = ordered_unkey(a.kmx[c]);
            o.centroid[c] = nan_centroid ? (double)NAN : (double)a.sum[c] / (double)o.count / REG_FIXED;
        }
    }
    const size_t k = std::min(cap, N);
    for (size_t i = 0; out_labels && i < k; ++i) {
        out_labels[i] = -1;
        if (owner[i] < 0) continue;
        const long long v = node_of((size_t)owner[i], labels[(size_t)owner[i]][i]);
        if (v < 0) return PPP_ERR_ARG; /* a label without its part row */
        out_labels[i] = acc[find((size_t)v)].label;
    }
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
    float mn[3], mx[3];
    if (ref->ranged) { for (int d = 0; d < 3; ++d) { mn[d] = ref->h_mn[d]; mx[d] = ref->h_mx[d]; } }
    else {
        rc = fetch_meta(ref);
        if (rc) return ref == h ? rc : fail(h, rc, std::string("registration tile: the reference: ") + ref->err);
        for (int d = 0; d < 3; ++d) { mn[d] = ref->hmeta.mn[d]; mx[d] = ref->hmeta.mx[d]; }
    }
    double ext[3];
    for (int d = 0; d < 3; ++d) {
        F.c[d] = ((double)mn[d] + (double)mx[d]) * 0.5;
        ext[d] = (double)mx[d] - (double)mn[d];
    }
    F.Ln = (((ext[0] + ext[1]) + ext[2]) * 0.5) + (double)P.max_dist;
    F.scale = std::ldexp(1.0, shift);
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

/* the wait for a tile's evaluation, and its row: the refusal (B.89), the words' sanity, the terms */
static int regt_collect(RegtTile &t, const double *T, ppp_registration_row *row)
{
    ppp_handle h = t.h;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const unsigned long long *w = h->registration.tpin.p;
    if (w[REGT_REFUSED])
        return fail(h, PPP_ERR_CAPACITY, "registration tile: " + std::to_string(w[REGT_REFUSED]) + " moved queries reach beyond the reference's indexed slice range "
                    "(max_dist + normal_radius around the moved point): raise range_margin of the reference's handle");
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
    int rc = registration_params_ok(h, *rp, F);
    if (rc) return rc;
    static const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(T, T0 ? T0 : I, sizeof(I));
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) return fail(h, PPP_ERR_ARG, "registration tile: the transform has an entry that is not finite");
    return PPP_OK;
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
    static const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    *out_row = ppp_registration_row{};
    icp_row_terms(out_row, T12 ? T12 : I, acc);
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

/* the tiles' rows of one evaluation at T as the whole cloud's (B.91), with the checks the loops make of it */
static int regt_merged(ppp_handle h0, const std::vector<ppp_registration_row> &part_rows, const std::vector<ppp_registration_part> &parts, const double *T,
                       ppp_registration_row &rw, ppp_registration_part &whole)
{
    const int rc = ppp_merge_registration_terms(part_rows.data(), parts.data(), parts.size(), T, &rw, &whole);
    if (rc) return fail(h0, rc, "registration tiles: the tiles' ranges overlap, or the tiles do not hold one scan against one reference");
    if (rw.pairs > whole.owned) return fail(h0, PPP_ERR_HIP, "registration tiles: sums corrupt");
    return PPP_OK;
}

/* ppp_register's statistics from a tiled loop's rows */
static ppp_registration_stats regt_stats(const std::vector<ppp_registration_row> &R, const IcpCtl &C, const ppp_registration_part &whole)
{
    const size_t last = (size_t)C.steps;
    ppp_registration_stats st = {};
    st.n = whole.n; st.indexed = whole.owned;
    st.steps = C.steps; st.converged = C.converged; st.locked = C.locked; st.shift = whole.shift;
    for (int d = 0; d < 3; ++d) st.centre[d] = whole.centre[d];
    st.length = whole.length;
    memcpy(st.T, R[last].T, sizeof(st.T));
    auto rms = [&](const ppp_registration_row &r) {
        return r.pairs ? std::sqrt(std::ldexp((double)r.E, -whole.shift) / (double)r.pairs) : (double)NAN;
    };
    st.pairs_before = R[0].pairs; st.rms_before = rms(R[0]);
    st.pairs_after = R[last].pairs; st.rms_after = rms(R[last]);
    return st;
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
    if (!rows && row_cap) return fail(h0, PPP_ERR_ARG, "registration tiles: rows is NULL with row_cap > 0");
    for (size_t i = 0; i < count; ++i) {
        if (!hs[i] || !refs[i]) return fail(h0, PPP_ERR_ARG, "registration tiles: a NULL handle");
        for (size_t k = 0; k < i; ++k) if (hs[k] == hs[i]) return fail(h0, PPP_ERR_ARG, "registration tiles: a scan handle stands in two slots");
    }
    const ppp_registration_params P = *rp;
    auto failed = [&](size_t i, int code) { if (stats) stats->failed_tile = (int)i; return code; };
    std::vector<RegtTile> tiles(count);
    for (size_t i = 0; i < count; ++i) {
        tiles[i].h = hs[i]; tiles[i].ref = refs[i];
        bool first = true; /* the reference's index and normal field: once per reference handle */
        for (size_t k = 0; k < i; ++k) first = first && refs[k] != refs[i];
        rc = regt_prepare(tiles[i], P, F, first);
        if (rc) return failed(i, rc);
    }
    std::vector<ppp_registration_row> part_rows(count), R;
    std::vector<ppp_registration_part> parts(count);
    ppp_registration_part whole = {};
    IcpCtl C = {};
    rc = regt_loop(P, F, T, R, C, whole, [&](int, ppp_registration_row &rw) {
        for (size_t i = 0; i < count; ++i) { int e = regt_enqueue(tiles[i], T); if (e) return failed(i, e); }
        int first_rc = PPP_OK;
        size_t first_at = 0;
        for (size_t i = 0; i < count; ++i) { /* every tile is waited for, whatever an earlier one answered */
            const int e = regt_collect(tiles[i], T, &part_rows[i]);
            if (e && !first_rc) { first_rc = e; first_at = i; }
            parts[i] = tiles[i].part;
        }
        if (first_rc) return failed(first_at, first_rc);
        return regt_merged(h0, part_rows, parts, T, rw, whole);
    });
    if (rc) return rc;
    if (stats) stats->reg = regt_stats(R, C, whole);
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

static int trimt_wait(RegtTile &t)
{
    HIPCHK(t.h, hipSetDevice(t.h->device));
    HIPCHK(t.h, hipStreamSynchronize(t.h->stream));
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
    if (!rows && row_cap) return fail(h0, PPP_ERR_ARG, "trimmed registration tiles: rows is NULL with row_cap > 0");
    for (size_t i = 0; i < count; ++i) {
        if (!hs[i] || !refs[i]) return fail(h0, PPP_ERR_ARG, "trimmed registration tiles: a NULL handle");
        for (size_t k = 0; k < i; ++k) if (hs[k] == hs[i]) return fail(h0, PPP_ERR_ARG, "trimmed registration tiles: a scan handle stands in two slots");
    }
    const ppp_registration_params P = tp->icp;
    auto failed = [&](size_t i, int code) { if (stats) stats->failed_tile = (int)i; return code; };
    auto map_of = [&](auto *const *maps, size_t i) { return maps ? maps[i] : nullptr; };
    std::vector<RegtTile> tiles(count);
    for (size_t i = 0; i < count; ++i) {
        tiles[i].h = hs[i]; tiles[i].ref = refs[i];
        bool first = true; /* the reference's index and normal field: once per reference handle */
        for (size_t k = 0; k < i; ++k) first = first && refs[k] != refs[i];
        rc = regt_prepare(tiles[i], P, F, first);
        if (!rc) rc = trimt_prepare(tiles[i], map_of(status, i) || map_of(d2, i) || map_of(owned, i));
        if (rc) return failed(i, rc);
    }
    /* every tile is waited for, whatever an earlier one answered; the first error is the call's */
    auto wait_all = [&]() {
        int first_rc = PPP_OK;
        for (size_t i = 0; i < count; ++i) {
            const int e = trimt_wait(tiles[i]);
            if (e && !first_rc) first_rc = failed(i, e);
        }
        return first_rc;
    };
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
    std::vector<ppp_registration_row> part_rows(count), R;
    std::vector<ppp_registration_part> parts(count);
    ppp_registration_part whole = {};
    IcpCtl C = {};
    rc = regt_loop(P, F, T, R, C, whole, [&](int, ppp_registration_row &rw) {
        for (size_t i = 0; i < count; ++i) { const int e = trimt_enqueue_pair(tiles[i], T); if (e) return failed(i, e); }
        int e = wait_all();
        if (e) return e;
        size_t paired = 0;
        for (size_t i = 0; i < count; ++i) {
            RegtTile &t = tiles[i];
            const unsigned *w = trimt_pinned_hist(t);
            if (w[TRIMT_REFUSED])
                return failed(i, fail(t.h, PPP_ERR_CAPACITY, "trimmed registration tiles: " + std::to_string(w[TRIMT_REFUSED]) + " moved queries reach beyond the "
                                      "reference's indexed slice range (max_dist + normal_radius around the moved point): raise range_margin of the "
                                      "reference's handle"));
            size_t mine = 0;
            for (size_t b = 0; b < TRIM_B0; ++b) mine += w[TRIMT_HEAD + b];
            if (w[TRIMT_OWNED] > (unsigned)trimt_positions(t) || mine > w[TRIMT_OWNED]) return failed(i, fail(t.h, PPP_ERR_HIP, "trimmed registration tiles: histogram corrupt"));
            t.part.owned = w[TRIMT_OWNED];
            parts[i] = t.part;
            part_rows[i] = ppp_registration_row{};
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
                for (size_t i = 0; i < count; ++i) { e = trimt_enqueue_narrow(tiles[i], pass, prefix); if (e) return failed(i, e); }
                e = wait_all();
                if (e) return e;
                merge_hist(0, bins);
                ppp_trim_select(H.data(), bins, rank, &bin, &rank);
                if (!rank) return fail(h0, PPP_ERR_HIP, "trimmed registration tiles: cut corrupt");
                prefix |= pass == 1 ? bin << 10 : bin;
            }
            cut.tau = prefix;
            for (size_t i = 0; i < count; ++i) { e = trimt_enqueue_terms(tiles[i], cut.tau); if (e) return failed(i, e); }
            e = wait_all();
            if (e) return e;
            for (size_t i = 0; i < count; ++i) {
                const unsigned long long *w = tiles[i].h->registration.tpin.p;
                if (w[ICP_PAIRS] > parts[i].owned) return failed(i, fail(tiles[i].h, PPP_ERR_HIP, "trimmed registration tiles: sums corrupt"));
                icp_row_terms(&part_rows[i], T, w);
            }
        }
        e = regt_merged(h0, part_rows, parts, T, rw, whole);
        if (e) return e;
        if (rw.pairs > paired || (paired && rw.pairs < trim_rank(keep, paired))) return fail(h0, PPP_ERR_HIP, "trimmed registration tiles: cut corrupt");
        cuts.push_back(cut);
        return (int)PPP_OK;
    });
    if (rc) return rc;
    const size_t last = (size_t)C.steps;
    /* B.99: the maps of the last evaluation -- its keys are the ones the tiles hold --, every tile's launch before any copy */
    for (size_t i = 0; i < count; ++i)
        if (map_of(status, i) || map_of(d2, i) || map_of(owned, i)) {
            rc = trimt_enqueue_scatter(tiles[i], cuts[last].tau, cuts[last].paired == 0);
            if (rc) return failed(i, rc);
        }
    for (size_t i = 0; i < count; ++i) {
        rc = trimt_copy_maps(tiles[i], map_of(status, i), map_of(d2, i), map_of(owned, i), cap);
        if (rc) return failed(i, rc);
    }
    if (stats) stats->reg = regt_stats(R, C, whole);
    const size_t k = std::min(row_cap, last + 1);
    for (size_t i = 0; rows && i < k; ++i) {
        ppp_trimmed_registration_row &o = rows[i];
        memset(&o, 0, sizeof(o)); /* the padding too: rows compare as bytes */
        o.row = R[i];
        o.paired = cuts[i].paired;
        memcpy(&o.trim_d2, &cuts[i].tau, sizeof(float));
    }
    return PPP_OK;
}

} // extern "C"
