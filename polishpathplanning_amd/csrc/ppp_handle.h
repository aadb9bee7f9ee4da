/*
 * ppp_handle.h -- what the host units of the engine share: the handle (ppp_handle_s) and the types it is made of, the launch
 * geometry of a slab pass, a batch graph, the HIPCHK / LAUNCH macros, and the declarations of the helpers that more than one
 * unit calls.  Internal: nothing of it is part of the C ABI (include/ppp_hip.h).
 *
 *   ppp_engine.hip   the handle, the plan and the passes, graphs and batches, the getters and the API mirrors; it defines
 *                    every helper declared here
 *   ppp_contact.hip  the contact queries: coverage, path coverage, path contacts, the contact field, the regions, the schedules
 *   ppp_scan.hip     the calls that hold a scan against a reference cloud: the deviation map, the registrations, their tiles;
 *                    the resident triangle mesh and the exact deviation against it
 *   ppp_preproc.hip  the four preprocessing calls on the resident cloud, and the mesh sampler that makes one (ppp_set_cloud_mesh)
 *
 * A helper that only one unit calls is static in that unit and is not declared here.
 */
#pragma once
#include "ppp_window_decl.h" /* WinArgs (ppp_kernels.h with it) */
#include "ppp_dynamic.h"     /* DynParams */
#include "ppp_compact.h"
#include "ppp_sort.h"
#include "../../include/ppp_hip.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

struct RegAcc; /* ppp_regions.h: a region's accumulators (the handle owns buffers of them; only the contact unit looks inside) */
struct FeedRec; /* ppp_feed.h: what the feed envelope reads of a waypoint (likewise) */
struct IcpFrame; /* ppp_registration.h: what does not change along a registration chain (only the scan unit looks inside) */

/* The types and helpers of the host units.  Hidden: the library is linked without visibility flags, and names like `fail` or
   `compact` are not for its dynamic symbol table. */
namespace ppp_internal __attribute__((visibility("hidden"))) {

struct KTimer {
    std::string name;
    std::vector<hipEvent_t> e0, e1; /* one pair per launch of this kernel in a pass */
    int used = 0;
};

/* memory owned by one object: ensure() grows it (the contents are not kept), release() frees it early, the destructor
   frees it.  Move-only.  Device memory (DevBuf) or pinned host memory (PinBuf). */
template <typename T, bool PINNED>
struct OwnedBuf {
    T *p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~OwnedBuf() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= cap && p) return hipSuccess;
        release();
        if (n == 0) n = 1;
        hipError_t e = PINNED ? hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
};
template <typename T> using DevBuf = OwnedBuf<T, false>;
template <typename T> using PinBuf = OwnedBuf<T, true>;

/* where the meta block of the pass just enqueued will turn up on the host */
struct MetaAt {
    enum Kind { ON_DEMAND /* nowhere: copied when somebody asks */, PINNED /* the handle's hmeta_pinned */, BATCH_SLOT /* entry slot of a batch's pinned array */ };
    Kind kind = ON_DEMAND;
    std::shared_ptr<PinBuf<DevMeta>> batch; /* batched launches publish every member's meta block in one pinned array, shared with the members that read it */
    size_t slot = 0;
    static MetaAt on_demand() { return MetaAt(); }
    static MetaAt pinned() { MetaAt a; a.kind = PINNED; return a; }
    static MetaAt batch_slot(const std::shared_ptr<PinBuf<DevMeta>> &metas, size_t i) { MetaAt a; a.kind = BATCH_SLOT; a.batch = metas; a.slot = i; return a; }
};

/* What a handle knows about its plan and its last pass.  The members change only through the transitions below, each named
   for what happened on the handle; the queries' caches (coverage, contacts, regions, the knots' host copy) key on serial(). */
class PassState {
    bool planned_ = false, index_built_ = false, gen_done_ = false, path_done_ = false;
    bool list_final_ = false;    /* wp_out holds a finished WayPointsList */
    bool stage_compact_ = true;  /* wp_xyz / wp_nn / wp_normal hold the list order (a window pass leaves them in per-slice slots) */
    bool finish_lists_stale_ = false; /* wp_pre / wp_smooth are an earlier pass's: the window path's finish launch writes them only for a pass enqueued call by call */
    unsigned long long serial_ = 0; /* counts the GenPaths enqueued */
    bool meta_fresh_ = false;    /* hmeta is the device's block as of now: nothing was launched on this handle since it was fetched (every launch clears it) */
    MetaAt meta_at_;             /* where the copy enqueued behind the last pass lands (ON_DEMAND: none was enqueued) */
    hipStream_t pending_stream_ = nullptr; /* a batch graph launched on another handle's stream carries this handle's work */
    void withdraw_results() { index_built_ = false; gen_done_ = false; meta_fresh_ = false; path_done_ = false; list_final_ = false; }

public:
    bool planned() const { return planned_; }
    bool index_built() const { return index_built_; }
    bool gen_done() const { return gen_done_; }
    bool path_done() const { return path_done_; }
    bool list_final() const { return list_final_; }
    bool stage_compact() const { return stage_compact_; }
    bool finish_lists_stale() const { return finish_lists_stale_; }
    unsigned long long serial() const { return serial_; }
    bool meta_fresh() const { return meta_fresh_; }
    bool meta_in_flight() const { return meta_at_.kind != MetaAt::ON_DEMAND; }
    /* the block the copy in flight lands in (handle_block: the handle's own pinned one) */
    const DevMeta *meta_landing(const DevMeta *handle_block) const
    {
        return (meta_at_.kind == MetaAt::BATCH_SLOT && meta_at_.batch) ? meta_at_.batch->p + meta_at_.slot : handle_block;
    }
    hipStream_t pending_stream() const { return pending_stream_; }

    /* no plan, no index, no results */
    void withdraw_plan() { planned_ = false; withdraw_results(); }
    void plan_made() { stage_compact_ = true; planned_ = true; withdraw_results(); }
    /* a cloud was set without waiting for its bounds: results and index are gone, the plan stays */
    void cloud_replaced_under_plan() { withdraw_results(); }
    void index_enqueued() { index_built_ = true; }
    void gen_enqueued(bool window) { if (window) stage_compact_ = false; gen_done_ = true; ++serial_; path_done_ = false; }
    /* getPath (a window pass's stage lists stay as they are: still in slots, or gathered since) */
    void path_enqueued(bool final, bool window, bool finish_lists = true)
    {
        path_done_ = true; list_final_ = final; finish_lists_stale_ = !finish_lists;
        if (!window) stage_compact_ = true;
    }
    /* GenPath and getPath at once (a graph launch); carrier: the other handle's stream the work runs on */
    void pass_enqueued(bool window, bool final, MetaAt at, hipStream_t carrier = nullptr)
    {
        if (!window) index_built_ = true;
        stage_compact_ = !window;
        finish_lists_stale_ = window && final; /* (a slice-range handle's finish launch stops at wp_pre and always writes it) */
        gen_done_ = true; ++serial_; path_done_ = true;
        list_final_ = final;
        meta_will_arrive(std::move(at));
        pending_stream_ = carrier;
    }
    /* a new plan turned out to ask for the very launches the last pass ran: its results stand */
    void restore_results(bool had_path, bool was_final) { gen_done_ = true; path_done_ = had_path; list_final_ = was_final; }
    void stages_gathered() { stage_compact_ = true; }
    void finish_lists_made() { finish_lists_stale_ = false; }
    void streams_settled() { pending_stream_ = nullptr; }
    /* (a batch's pinned array stays referenced until a later batch's takes its place, whatever arrives in between: no getter
       ends up freeing pinned memory) */
    void meta_will_arrive(MetaAt at)
    {
        if (at.kind == MetaAt::BATCH_SLOT) meta_at_ = std::move(at); else meta_at_.kind = at.kind;
        meta_fresh_ = false;
    }
    void meta_stale() { meta_fresh_ = false; }
    void meta_read() { meta_at_.kind = MetaAt::ON_DEMAND; meta_fresh_ = true; }
};

} // namespace ppp_internal
using namespace ppp_internal;

struct ppp_handle_s {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    ppp_params P;
    float vp[3] = {0, 0, 0};
    size_t n = 0;
    bool have_cloud = false;
    PassState pass; /* the plan and the last pass: what is planned, built, enqueued, and where its meta block arrives */
    /* host copy of the knots of the last pass (slice tables + node arrays), fetched whole by the first ppp_get_nodes after a pass:
       the planner classes ask slice by slice (a Spline view per slice: 2 calls x 256 slices), and a synchronous copy of a few
       bytes costs ~20 us on this runtime -- 60 ms of GenPath() for 0.07 ms of planning before this cache */
    unsigned long long hn_serial = ~0ull; /* the pass (pass.serial()) the copy belongs to */
    std::vector<int> hn_off;    /* S + 1 offsets into ... */
    std::vector<float> hn_xyz;  /* ... three planes (x | y | z) of hn_off[S] floats */
    DevBuf<int> pack_tab;       /* device: node_start as the host validated it, then the offsets */
    DevBuf<float> pack_out;
    int max_lds = 65536;
    int num_cus = 256;

    /* plan */
    int B = 1, slab_cap = 4096, S_cap = 1, capb = 2048, W_cap = 1, node_cap = 1;
    int knot_cap = 2048, stage_cap = POSE_STAGE_CAP, tab_slabs = 8, pose_threads = POSE_T, cnt_est = 1; /* launch geometry of k_pose (make_plan) */
    float pose_pad = 8.f;
    float h_mn[3] = {0, 0, 0}, h_mx[3] = {0, 0, 0};
    int h_nvalid = 0;
    /* slice-range handles (SURVEY.md 8e case ii) */
    bool ranged = false;          /* plans a strict sub-range of the slices: getPath stops after a12 */
    /* trans2center ran (Alignment = true): TransAlign, its inverse, and a second handle holding the cloud carried back by
       the inverse with its own slab index (path_translation_alg.cpp:171-174 searches and estimates normals there) */
    bool aligned = false;
    float TA[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}}, invTA[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    ppp_handle back = nullptr;
    int sb = 0, se = 0;           /* the range, resolved against the walk */
    float incl_lo = -INFINITY, incl_hi = INFINITY;
    int n_range = 0;              /* expected number of indexed points */

    DevBuf<float> X, Y, Z;
    /* slice-range handles: the points of [incl_lo, incl_hi] in cloud order with their cloud indices (built by make_plan):
       the hot path streams these instead of the whole cloud */
    DevBuf<float> Xp, Yp, Zp;
    DevBuf<int> part_idx;
    int n_part = 0;
    bool use_part = false;
    /* ppp_set_cloud_part: the resident cloud IS a part (every point with x in [part_lo, part_hi], cloud order); the whole
       cloud's bounds and point count came with it, part_idx (optional) holds the points' cloud indices */
    bool part_given = false;
    bool part_has_idx = false;
    float part_lo = 0.f, part_hi = 0.f;
    DevBuf<float4> unsorted4, sorted4;
    DevBuf<int> slab_cnt, slab_start, slab_cursor, coarse_cursor, slab_ytab;
    bool two_pass_scatter = false; /* large clouds: coarse bins first (see k_slab_scatter) */
    DevBuf<float> slab_xmin, slab_xmax;
    DevBuf<DevMeta> meta;
    DevBuf<float> px, lo, hi;
    DevBuf<float> node_x, node_y, node_z;
    /* dynamic adjustment (allocated when Dynamic_adjustment is on or ppp_area2cloud is used) */
    DevBuf<float4> normals4, dyn_bnd_pts, dyn_adj_pts, dyn_first_ab, dyn_first_snap;
    DevBuf<double> dyn_first_node;
    DevBuf<float> ell_cs;
    DevBuf<double> dyn_bnd_knots;
    DevBuf<int> dyn_bnd_n;
    int dyn_maxNB = 1, dyn_maxNA = 1;
    bool dyn_keep_all = false;
    DevBuf<int> dyn_raw_sc;           /* [slice][2]: node_start / node_cnt as fitted, before the chain (k_dyn_first_eval) */
    /* coverage of the last pass (ppp_get_coverage): flags by cloud index, zero-padded to 16 bytes, and the covered count */
    /* path coverage of the last pass (ppp_get_path_coverage): the same, for the final paths of every walk; [1] of the count
       buffer holds the kernel's refusals (1: a search left the indexed slice range, 2: a knot table out of bounds) */
    struct FlagCoverage { DevBuf<unsigned char> flags; DevBuf<int> count; unsigned long long serial = ~0ull /* the pass (pass.serial()) they belong to */; size_t covered = 0; } cov, pcov;
    /* path contacts of the last pass (ppp_get_path_contacts): the maps by cloud index, the per-slice sample table (rows from
       off; its last two entries the row count and k_pcon_offsets's refusals), the slices' reach keys and the statistics
       (acc: bins, covered, multi_slice, total, max, the refusal word; the int at acc + 69 is where the kernels set it) */
    struct PathContacts {
        DevBuf<unsigned> counts, reach;
        DevBuf<int> first, last, off;
        DevBuf<float4> tab;
        DevBuf<unsigned long long> acc;
        unsigned long long serial = ~0ull;
        ppp_contact_stats stats = {};
        /* the sample table alone (off, tab, reach), which ppp_get_path_removal shares: the pass it belongs to -- set once a
           caller has read the sample kernels' refusal word back clean -- the first slice, the slices and the rows it holds */
        unsigned long long tab_serial = ~0ull;
        int tab_sb = 0, tab_nsl = 0, tab_rows = 0;
    } pcon;
    /* predicted removal of the last pass (ppp_get_path_removal): per table row the path length its sample stands for and per
       slice their sum (ds_serial: the pass), the held flags by cloud index (the same for every profile, written by each map's
       launch), the statistics' accumulators, and per profile the map by cloud index with its statistics */
    struct PathRemoval {
        DevBuf<double> ds, slice_len, psum;
        DevBuf<unsigned char> held;
        DevBuf<unsigned long long> acc;
        unsigned long long ds_serial = ~0ull;
        double path_length = 0.0;
        struct Slot { DevBuf<double> map; unsigned long long serial = ~0ull; ppp_removal_stats stats = {}; } slot[3];
    } prem;
    /* dwell schedule of the last pass (ppp_get_path_dwell): per table row the factor t, the scaled length dst = ds * t and the
       fixed-point sums num / den of the transposed walk; by cloud index the ratio g, the caller's target and the map the factors
       predict -- maps of its own: prem's unit-feed maps stay as they are.  The result of a call without a target is kept for
       (serial, profile, iterations, dmin, dmax): rows and stats on the host, the map on the device. */
    struct PathDwell {
        DevBuf<double> t, dst, g, target, map, psum;
        DevBuf<long long> num, den;
        DevBuf<unsigned long long> acc;
        bool valid = false;
        unsigned long long serial = ~0ull;
        int profile = 0, iterations = 0;
        double dmin = 0.0, dmax = 0.0;
        std::vector<ppp_dwell_row> rows;
        ppp_dwell_stats stats = {};
    } dwell;
    /* feed schedule of the last pass's WayPointsList (ppp_get_path_feed): the kept slices' offsets into the list and into the
       dwell rows, those rows' y and factors, the (slice, tile) list of the envelope's workgroups; per waypoint the cap, the
       segment's fixed-point length D, the envelope's record, the time ahead of it on its slice and the row; per kept slice
       the link's length and time, the slice's length and time.  The result of a call without a target is kept on the host for
       (serial, profile, iterations, dmin, dmax, the feed parameters). */
    struct PathFeed {
        DevBuf<int> off, rowoff;
        DevBuf<int2> tiles;
        DevBuf<float> ry;
        DevBuf<double> rt, cap;
        DevBuf<long long> D, tloc, linkD, linkT, slice_len, slice_t;
        DevBuf<FeedRec> rec;
        DevBuf<ppp_feed_row> rows;
        DevBuf<unsigned long long> acc;
        bool valid = false;
        unsigned long long serial = ~0ull;
        int profile = 0, iterations = 0;
        double dmin = 0.0, dmax = 0.0;
        ppp_feed_params fp = {};
        std::vector<ppp_feed_row> host_rows;
        ppp_feed_stats stats = {};
    } feed;
    /* deviation of this handle's cloud against another handle's (ppp_get_deviation): by cloud index the deviation, its local
       mean, its fixed-point term, the float d2, the reference index, the status and the target; the statistics' accumulators and
       the workgroups' parts of the two fixed-order sums.  Nothing is kept between calls: the reference may have changed.
       ppp_get_deviation_tile runs in the same buffers, with the owned map beside them; ppp_get_mesh_deviation too (ref_index
       holds the triangle), with the distance and region maps and the four words of their statistics beside them;
       ppp_get_mesh_signed_deviation adds the feature and flags maps and the five words of their counts. */
    struct Deviation {
        DevBuf<double> dev, smoothed, target, psum, dist;
        DevBuf<long long> fix;
        DevBuf<float> d2;
        DevBuf<int> ref_index;
        DevBuf<unsigned char> status, owned, region, feature, flags;
        DevBuf<unsigned long long> acc, macc, sacc;
    } deviation;
    /* registration of this handle's cloud to another handle's (ppp_get_registration_terms, ppp_register): the chain's transforms
       (12 doubles each), the 29 integer sums of every evaluation, the rows and the control words (IcpCtl, as ints).  Nothing is
       kept between calls. */
    struct Registration {
        DevBuf<double> T;
        DevBuf<unsigned long long> acc;
        DevBuf<ppp_registration_row> rows;
        DevBuf<int> ctl;
        /* ppp_get_cloud_moments: the ten words.  ppp_register_global's coarse stage: per start the transforms, sums, rows and
           control words of its chain, the compacted queries and the compaction's block counts and total */
        DevBuf<unsigned long long> mom, macc;
        DevBuf<double> mT;
        DevBuf<ppp_registration_row> mrows;
        DevBuf<int> mctl, qcnt;
        DevBuf<float4> queries;
        /* ppp_register_trimmed: per query in slab order the reference point of its pair and the key of the pair's d2 (the last
           evaluation's), per evaluation the three digit histograms and the cut (TrimCut, as words), and the two maps by cloud
           index.  ppp_register_mesh keeps the winning record of every query of the current evaluation in key */
        DevBuf<float4> partner;
        DevBuf<unsigned> key, hist, cuts;
        DevBuf<unsigned char> tstatus;
        DevBuf<float> td2;
        /* ppp_register_robust: with partner, key, hist, cuts, tstatus and td2 (the weight map) above, per query in slab order
           the residual of its pair, per evaluation sigma, and the residual map by cloud index */
        DevBuf<double> rres, rsigma, rresid;
        /* ppp_register_mesh_robust: with key, hist, cuts, the maps and the three above, per query in slab order the winning
           record of its pair (key holds the residual's key there, so the record needs room of its own) */
        DevBuf<unsigned> mwin;
        /* ppp_get_registration_terms_tile, ppp_register_tiles: the frame the tile's kernel reads, and pinned host memory for
           the transform on its way to the device and the words on their way back */
        DevBuf<IcpFrame> tframe;
        PinBuf<unsigned long long> tpin;
    } registration;
    /* contact field of the resident cloud (ppp_get_contact_field): the maps by cloud index and the statistics' accumulators;
       valid for P's contact parameters until the cloud changes (valid) */
    struct ContactField {
        DevBuf<float> curv, hw;
        DevBuf<unsigned long long> acc;
        DevBuf<double> psum;
        bool valid = false;
        unsigned long long built = 0; /* how many times the maps were computed: what a result derived from them belongs to */
        ppp_params P = {};
        float min_width = 0.f;
        ppp_contact_field_stats stats = {};
    } field;
    /* the contact field of the points this handle owns (ppp_get_contact_field_tile): the maps of the evaluated points by cloud
       index, hw_own = the half widths of the owned points alone (what the statistics read), the owned map, cnt = owned points,
       evaluated points, the refusal word; kept for P's contact parameters and range and for halo until the cloud changes */
    struct FieldTile {
        DevBuf<float> curv, hw, hw_own;
        DevBuf<unsigned char> owned;
        DevBuf<int> cnt;
        DevBuf<unsigned long long> acc;
        DevBuf<double> psum;
        bool valid = false;
        unsigned long long built = 0;
        ppp_params P = {};
        float halo = 0.f, min_width = 0.f;
        ppp_contact_field_tile_stats stats = {};
    } ftile;
    /* the regions of this handle's tile (ppp_get_regions_tile), as the call hands them out; the device work runs in `regions` */
    struct RegionTile {
        bool valid = false;
        int source = -1;
        float threshold = 0.f, link = 0.f;
        unsigned long long serial = 0;
        std::vector<int> labels;
        std::vector<ppp_region_part> parts;
        std::vector<ppp_region_halo> halos;
        ppp_region_tile_stats stats = {};
        DevBuf<unsigned char> owned; /* a MASK call's owned map (NARROW reads the field tile's: the same range and halo) */
        DevBuf<int> cnt;
    } rtile;
    /* connected regions (ppp_get_regions): the selection by slab-index position, the dense list of the selected positions and
       its inverse (ord), the union-find and the accumulators by ordinal, the labels by cloud index, the region rows in label
       order; tot: regions, singletons, largest, the refusal word, then the two compaction totals.  Kept for (source, threshold,
       link, serial of the source's result) */
    struct Regions {
        DevBuf<unsigned char> sel, mask;
        DevBuf<int> list, ord, parent, labels, head_root, cnt;
        DevBuf<RegAcc> acc, rows;
        DevBuf<unsigned> tot;
        bool valid = false, nan_centroid = false;
        int source = -1;
        float threshold = 0.f, link = 0.f;
        unsigned long long serial = 0;
        ppp_region_stats stats = {};
    } regions;
    DevBuf<int> node_start, node_cnt, band_cnt;
    DevBuf<int> wp_cnt, wp_off, tail, slice_wpcnt;
    DevBuf<float4> wp_xyz, wp_normal;
    DevBuf<int> wp_nn;
    DevBuf<float> wp_pre, wp_smooth, wp_out;
    DevBuf<MinMaxPart> mm_part;
    DevBuf<int> big_slabs, big_slices; /* work lists of the LDS-overflow fallback kernels */
    DevBuf<char> arena;                /* their global scratch, allocated on first need */
    bool big_path = false;             /* launch the fallback kernels (set by the plan or after an overflow) */
    int mm_grid = 1, sm_tiles = 1;
    DevBuf<char> scratch; /* API staging */
    /* window path (ppp_window.h): three launches, every point binned once into the window of its slice */
    bool win_allowed = true;    /* ppp_set_fast_path */
    bool win_disabled = false;  /* a pass was handed back (overflow / reach / stale plan): this cloud + parameters stay on the slab path */
    bool win_path = false;      /* the current plan runs the window path */
    bool win_staged = false;    /* the binning launch writes through LDS in window order (large clouds, ppp_window.h) */
    float win_pad = 4.f;
    int win_NBc_thr = 0; /* y-buckets per class in launches of several workgroups per CU: the most that cost no workgroup its place in the LDS */
    int win_capw = 0, win_cap_el = 0, win_NB = 0, win_NBc = 0, win_stride = 1, win_threads = 256, win_ppt = 4, win_gs = 1;
    int win_scat_threads = WSC_T; /* threads of a binning workgroup (win_pick_scatter: narrower where passes share the device) */
    int win_prio_finish = 0;      /* WinArgs.prio of the by-value finish launch (win_pick_prio: 0 for a pass alone) */
    int win_ppt_alone = 4;        /* points per thread of the 1024-thread form: what a batch falls back to whose members chose different forms */
    int win_rec_lds = 0; /* waypoint records parked in the slice workgroup's LDS (0: in global slots) */
    int win_nkept = 0, win_first_kept = 0, win_el_expect = 0;
    float win_px0 = 0.f;
    DevBuf<float> win_px;
    DevBuf<int> win_cnt;
    DevBuf<float4> win_pts;
    DevBuf<MinMaxPart> win_part;
    DevBuf<float4> wps_xyz, wps_normal, wps_rec;
    DevBuf<int> fin_ticket; /* arrivals of the window finish launch's workgroups (the last one publishes the meta block) */
    DevBuf<int> wps_nn;
    DevBuf<float> wps_pre;

    DevMeta hmeta;
    PinBuf<DevMeta> hmeta_pinned; /* the hot calls end with an async copy of the device meta into it */
    /* a new cloud's plan without the host in the middle: k_ingest_minmax's last workgroup reduces the bounds and walks the slices,
       k_win_census_auto counts the windows, both write their results to pinned memory (PlanAuto + plane table + census) */
    DevBuf<int> plan_ticket;         /* [2], zero between launches */
    DevBuf<PlanAuto> plan_auto;
    bool auto_valid = false;         /* the pinned census belongs to the cloud just set, with auto_S slices and auto_pad */
    /* Plan reuse: a planner that is fed one scan after the other plans clouds of one size with one set of parameters.  The first
       plan takes its window capacities from a census of that cloud; a later cloud with the same point count, parameters, slice
       count and pad inherits them (+4 %) and skips the census launch -- the pass itself detects a window that does not fit
       (WIN_FLAG_OVERFLOW), and the plan is then made again from a census of its own */
    bool plan_reuse = true;          /* ppp_set_plan_reuse */
    bool inh_valid = false;          /* the members below describe a census-based window plan of this handle */
    int inh_S = 0, inh_n = 0, inh_max_w = 0, inh_max_el = 0;
    float inh_pad = 0.f;
    ppp_params inh_P;
    bool auto_px_only = false;       /* the cloud just set brought walk + pad along (auto_S, auto_pad, pinned plane table), but no census */
    bool plan_inherited = false;     /* the current window plan's capacities are inherited */
    int auto_S = 0;
    float auto_pad = 0.f;
    bool slab_cnt_used = true;       /* a slab-path pass has been enqueued since the slab histogram was last cleared by the plan */
    PinBuf<char> pin;                /* pinned staging for the small copies of the plan (bounds partials, plane table, census) */
    PinBuf<char> pcd_stage[2];       /* ppp_set_cloud_pcd: two pinned pieces ... */
    hipEvent_t pcd_ev[2] = {nullptr, nullptr}; /* ... and the event behind each one's copy */
    /* A cloud set while the handle holds a window plan of an earlier cloud of the same size and parameters does not wait for its
       bounds: the conversion pass is enqueued, the plan stays, and the pass of the new cloud may be enqueued right
       behind it -- the device checks walk length, pad, bounds and capacities against the record that pass leaves, and hands a
       pass back whose plan does not fit.  plan_deferred: that record has not been read yet (resolve_deferred does, at the first
       call that is not one of the three enqueue-only entry points). */
    int side_by_side = 1; /* handles the caller runs side by side on this device (ppp_set_side_by_side): from two on the slice workgroups of small windows stay at 512 threads, from three on the binning launch of a large cloud takes its narrow form */
    bool plan_deferred = false, deferred_census = false;
    bool rec_current = false;   /* plan_auto holds the record of the resident cloud (it came through k_ingest_minmax and was not altered since) */
    bool plan_walk_ok = false;  /* the window plan's S, pad and plane table are the device's own, bit for bit (plan_window: census that came with the cloud, or inherited) */
    bool chain_calls = false;       /* GenPath is followed by getPath in the same enqueue: its meta copy is skipped */
    bool quiet_finish = false;      /* the window path's finish launch does not publish the meta block (a batch of one: fetched when somebody asks) */
    float *out2 = nullptr;          /* batched form: the emitting launch also writes the list here (at most out2_cap rows) */
    int out2_cap = 0;
    float *last_out2 = nullptr;     /* where the last batch put this handle's list: a re-run after an LDS overflow writes there too */
    int last_out2_cap = 0;
    int internal = 0;               /* > 0 while GenPath / getPath are enqueued on behalf of a batch or a re-run (keeps last_out2) */
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    unsigned epoch = 0;                 /* bumped whenever the launch sequence of this handle changes */
    unsigned graph_epoch_seen = ~0u;    /* ppp_run_async: the plan epoch of the last call (the first call of a plan runs eagerly) */
    struct BatchGraph *batches[2] = {nullptr, nullptr}; /* cached batch graphs (lead handle only): two, so a caller can
                                                           alternate between two destination buffers (double buffering) */
    int batch_next = 0;                                 /* slot the next new graph replaces */
    bool timing = false;
    std::vector<KTimer> timers;

    void drop_graph()
    {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        graph_exec = nullptr; graph = nullptr;
        ++epoch;
    }
    void drop_batch();
    /* the resident cloud changed: what was made of the old points goes, the contact field with it.  under_plan: the cloud was
       set without waiting for its bounds (refresh_bounds_and_plan), and the plan stays */
    void cloud_replaced(bool under_plan = false)
    {
        if (under_plan) pass.cloud_replaced_under_plan(); else pass.withdraw_plan();
        field.valid = false; ftile.valid = false; rtile.valid = false;
    }
    ~ppp_handle_s()
    {
        /* the members' buffers are freed after this body, on the device it selects (`back` lives on the same device) */
        (void)hipSetDevice(device);
        drop_graph();
        drop_batch();
        for (int b = 0; b < 2; ++b) if (pcd_ev[b]) (void)hipEventDestroy(pcd_ev[b]);
        for (auto &t : timers) { for (auto e : t.e0) (void)hipEventDestroy(e); for (auto e : t.e1) (void)hipEventDestroy(e); }
        if (stream) (void)hipStreamDestroy(stream);
        if (back) { delete back; back = nullptr; }
    }
};

/* Launch geometry of a slab pass: what the stage launches need beside the record (SlabArgs).  slab_geom decides it for ONE
   handle; a batch joins its members' and launches every stage once with the result.  The defaults are the floors a batch
   starts from. */
struct SlabGeom {
    float slab_x0 = 0.f, slab_invw = 0.f; /* the slab grid */
    int g_minmax = 1, g_scatter = 1, g_scatter2 = 1, g_sort = 1, g_slice = 1, g_pose = 1, g_smooth = 1; /* workgroups per stage (g_scatter2: the second level of the two-level scatter, 4 points per thread) */
    int first_slab = 0;         /* a slice-range handle sorts the g_sort slabs of its interval only */
    int ppt = 4;                /* points per scatter thread: 4, 8 or 16 */
    int B = 1, slab_cap = 2048, capb = 1024; /* slabs, points of a slab and of a band in LDS */
    bool full_slabs = false;    /* slabs beyond the planned 832 points: the sort's wide form */
    bool two_fit = true;        /* two slice workgroups' bands fit a CU's LDS */
    long long slices = 0;       /* slice workgroups of the launch */
    int pose_threads = 256;
    size_t pose_lds = 0;
    size_t hist_lds() const { return sizeof(int) * (size_t)B; }
    /* threads per slab: 256 while a slab holds the planned 832 points on average (more slabs in flight per CU: cfg 2 sorts in
       15.3 us against 17.0), SORT_T for the fuller slabs of clouds beyond the 8192-slab cap (cfg 5: 125 us against 157) */
    int sort_threads() const { return full_slabs ? SORT_T : 256; }
    size_t sort_lds() const { return (size_t)slab_cap * 12 + 16; }
    /* Threads of a k_slice_kd workgroup.  One workgroup per slice with the band in LDS: 1024 threads finish a slice soonest
       (one round of nearest-neighbour queries for bands of up to 2048 points), and that is what counts while the slices of a
       launch fit the GPU in one go.  With several times more slices than CUs (batches of workpieces) two 512-thread
       workgroups per CU get more slices through -- if two bands fit the CU's LDS. */
    int slice_threads(int num_cus) const { return (two_fit && slices >= 2LL * num_cus) ? 512 : SLICE_KD_T; }
    size_t slice_lds() const { return slice_kd_bytes(capb); }
    size_t brute_lds() const { return slice_lds_bytes(capb); } /* k_slice, the brute pairing's generic form */
    /* a batch: every stage is launched for its widest member (a narrower member's surplus workgroups leave at once) */
    void join(const SlabGeom &o)
    {
        g_minmax = std::max(g_minmax, o.g_minmax); g_scatter = std::max(g_scatter, o.g_scatter); g_sort = std::max(g_sort, o.g_sort);
        g_slice = std::max(g_slice, o.g_slice); g_pose = std::max(g_pose, o.g_pose); g_smooth = std::max(g_smooth, o.g_smooth);
        ppt = std::max(ppt, o.ppt); B = std::max(B, o.B); slab_cap = std::max(slab_cap, o.slab_cap); capb = std::max(capb, o.capb);
        full_slabs = full_slabs || o.full_slabs; two_fit = two_fit && o.two_fit;
        slices += o.slices; /* (summed: the two-workgroup rule looks at the launch, and the launch is the batch's) */
        pose_threads = std::max(pose_threads, o.pose_threads); pose_lds = std::max(pose_lds, o.pose_lds);
    }
};

struct BatchGraph {
    std::vector<ppp_handle> hs;
    std::vector<unsigned> epochs;
    float *dst = nullptr;
    std::vector<size_t> off, cap;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> join;
    /* batched form (one launch per stage over all members): the members' records and meta blocks */
    bool batched = false, eager = false; /* eager: launched directly every time (kernel timing), no graph */
    SlabGeom geom; /* launch geometry over all members (slab path) */
    DevBuf<SlabArgs> members;
    bool win = false;              /* every member runs the window path: the three k_win_*_b launches */
    bool solo = false;             /* ONE window-path member: its own three launches with the arguments by value (no record, no meta array) */
    DevBuf<WinArgs> wmembers;
    int win_ppt = 4, win_scat_threads = WSC_T, win_threads = 256, gx_scat = 1, gx_slice = 1, gx_wfin = 1;
    bool win_staged = false;
    size_t win_lds = 0, win_scat_lds = 0, win_fin_lds = 0;
    DevBuf<DevMeta> metas;
    std::shared_ptr<PinBuf<DevMeta>> hmetas; /* the meta blocks on the host, shared with the member handles that read them */
    ~BatchGraph()
    {
        if (ge) (void)hipGraphExecDestroy(ge);
        if (g) (void)hipGraphDestroy(g);
        if (fork) (void)hipEventDestroy(fork);
        for (auto e : join) if (e) (void)hipEventDestroy(e);
    }
};

/* Seven helpers of the host side have always been dynamic symbols of the library under their plain names (index_ready,
   rebuild_back, cloud_changed, preproc_begin, adopt_cloud, enqueue_finish, read_piece: defined in an unnamed namespace inside
   extern "C").  The exported set is not this header's to change, so the one of them that a second unit calls keeps its name:
   the slab index of a handle, complete (ppp_engine.hip) */
extern "C" int index_ready(ppp_handle h, bool strict = true);

namespace ppp_internal __attribute__((visibility("hidden"))) {

/* ---- defined in ppp_engine.hip, called by the other units too ---- */
int fail(ppp_handle h, int code, const std::string &msg);
hipError_t copy_sync(ppp_handle h, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
KTimer *timer_for(ppp_handle h, const char *name);
int curvature_k_ok(ppp_handle h, int k);
DynParams dyn_params(const ppp_handle h);
int ensure_dynamic_buffers(ppp_handle h);
int enqueue_normals(ppp_handle h);
SlabGeom slab_geom(const ppp_handle h);
int settle(ppp_handle h);
int fetch_meta(ppp_handle h);
int map_dev_err(ppp_handle h);
int ensure_ready(ppp_handle h, bool need_gen, bool need_path);
int plan_ready(ppp_handle h);
int refresh_bounds_and_plan(ppp_handle h, const char *raw = nullptr, size_t stride_bytes = 0, bool may_defer = false, bool resident = false);
/* ppp_set_cloud_device for points that are in resident units already (the mesh sampler's): the same conversion pass, without its x1000 */
int set_cloud_resident(ppp_handle h, const float *xyz_dev, size_t n, const float *viewpoint);

#define HIPCHK(h, expr)                                                                               \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(h, PPP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)

/* launch helper: optional hipEvent bracket on the handle's stream */
#define LAUNCH(h, name, kern, grid, block, shmem, ...)                                                \
    do {                                                                                              \
        KTimer *_t = (h)->timing ? timer_for((h), name) : nullptr;                                    \
        if (_t) (void)hipEventRecord(_t->e0[_t->used], (h)->stream);                                  \
        (void)hipGetLastError(); /* the check below must not pick up an older, unrelated error */     \
        (h)->pass.meta_stale();                                                                       \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), (shmem), (h)->stream, __VA_ARGS__);         \
        if (_t) { (void)hipEventRecord(_t->e1[_t->used], (h)->stream); _t->used++; }                  \
        hipError_t _le = hipGetLastError();                                                           \
        if (_le != hipSuccess) return fail((h), PPP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(_le)); \
    } while (0)

/* a device-wide exclusive scan (ppp_sort.h) on the handle's stream, under its kernel timers like a launch; tmp: the scan's scratch */
static inline int scan_exclusive(ppp_handle h, const char *name, DevBuf<char> &tmp, const unsigned *in, unsigned *out, size_t n)
{
    size_t bytes = 0;
    HIPCHK(h, ppp_scan_exclusive_u32(nullptr, &bytes, in, out, n, h->stream));
    HIPCHK(h, tmp.ensure(bytes));
    KTimer *t = h->timing ? timer_for(h, name) : nullptr;
    if (t) (void)hipEventRecord(t->e0[t->used], h->stream);
    const hipError_t e = ppp_scan_exclusive_u32(tmp.p, &bytes, in, out, n, h->stream);
    if (t) { (void)hipEventRecord(t->e1[t->used], h->stream); t->used++; }
    HIPCHK(h, e);
    return PPP_OK;
}

/* Launch-geometry / search-radius overrides of the tuning scripts (tools/_run_*.sh): read only by builds made with -DPPP_TUNING
   (make variant NAME=tune DEFS=-DPPP_TUNING); the product library ignores them, so a stray variable cannot change a plan. */
static inline const char *tuning_env(const char *name)
{
#ifdef PPP_TUNING
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

/* the cuts of ownership: [cut(sb), cut(se)) of the walk px[0 .. S), the midpoints of neighbouring slices in float */
inline void owned_cuts(const float *px, int S, int sb, int se, float *own_lo, float *own_hi)
{
    if (sb >= se) { *own_lo = INFINITY; *own_hi = -INFINITY; return; } /* an empty range owns nothing */
    *own_lo = sb <= 0 ? -INFINITY : (px[sb - 1] + px[sb]) * 0.5f;
    *own_hi = se >= S ? INFINITY : (px[se - 1] + px[se]) * 0.5f;
}

/* ordered compaction (ppp_compact.h) of the n elements sel keeps: the block counts in cnt[0 .. n / COMPACT_CHUNK], their
   scan (the kept total to *total, on the device), the emit.  sized (the range part, whose output is sized by the total):
   the total is read back first, and sized(total) may point sel at the output before the emit. */
template <class Sel>
int compact(ppp_handle h, Sel &sel, int n, int *cnt, int *total, const std::function<int(int)> &sized = nullptr)
{
    const int nblocks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
    LAUNCH(h, "k_compact_count", k_compact_count<Sel>, nblocks, 256, 0, sel, n, cnt);
    LAUNCH(h, "k_compact_scan", k_compact_scan, 1, 1024, 0, cnt, nblocks, total);
    if (sized) {
        int kept = 0;
        HIPCHK(h, hipMemcpyAsync(&kept, total, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (int rc = sized(kept)) return rc;
    }
    LAUNCH(h, "k_compact_emit", k_compact_emit<Sel>, nblocks, 256, 0, sel, n, cnt);
    return PPP_OK;
}

} // namespace ppp_internal
