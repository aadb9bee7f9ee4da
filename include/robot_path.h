/*
 * robot_path.h -- drop-in for the reference's include/robot_path.h (class RobotPath, :58-98).
 * The reference header does not compile (its constructor is mis-named SectPath, :61-65) and no
 * .cpp implements it; its member list is the July snapshot src/path_connect_ex0720.cpp:
 * single-direction float walk from min.x + Radius, +-5 mm trim, no first/last drop, no position
 * smoothing, hand-eye constants of robot_path.h:36-41.  That behaviour is what this class runs.
 */
#ifndef ROBOT_PATH_H
#define ROBOT_PATH_H

#include <string>
#include <vector>
#include "Spline.h"

class RobotPath {
public:
    RobotPath() {}
    RobotPath(std::string configName, std::string CloudFileName, double Radius) : cloud_name(CloudFileName)
    {
        ppp_read_config(configName.c_str(), &planner.config());
        ppp_params &p = planner.config().params;
        p.tool_radius = Radius; p.pairing = PPP_PAIR_KD; p.walk = PPP_WALK_V1_CONTACT;
        p.trim = 5; p.drop_ends = 0; p.smooth = 0; /* path_connect_ex0720.cpp:440-448 */
        const float he[6] = {0.792078f, -0.042662f, 0.6656017f, -3.1531625f, -0.048573f, 1.609157f};
        for (int i = 0; i < 6; ++i) p.handeye[i] = he[i];
        planner.open(cloud_name);
    }
    void show() { planner.show_notice(); }
    void estimate_normal() { planner.estimate_normal(); } /* path_connect_ex0720.cpp: pcl::NormalEstimation, whole cloud */
    const std::vector<float> &cloud_normals() const { return planner.cloud_normals(); }
    void GenPath()
    {
        if (!planner.gen_path()) return;
        Path_set.clear();
        for (int s = 0; s < planner.num_slices(); ++s) Path_set.emplace_back(planner.handle(), s);
    }
    void getPath()
    {
        std::vector<float> wp;
        if (!planner.get_path(wp)) return;
        WayPointsList.assign(wp.size() / 6, std::vector<float>(6));
        for (size_t w = 0; w < WayPointsList.size(); ++w)
            for (int d = 0; d < 6; ++d) WayPointsList[w][d] = wp[6 * w + d];
    }
    const std::vector<std::vector<float>> &waypoints() const { return WayPointsList; }
    /* get_coverage's two lines (Path_Generation.cpp:766-770) for the planned paths (ppp_get_path_coverage) */
    void get_path_coverage() { planner.print_path_coverage(); }
    /* the contact counts of the planned paths: largest and mean, and the slices' overlap (ppp_get_path_contacts) */
    void get_path_contacts() { planner.print_path_contacts(); }
    /* how much the planned paths take off and how evenly: touched points, path length, mean / min / max removal and cv with the
       Hertzian profile (ppp_get_path_removal) */
    void get_path_removal() { planner.print_path_removal(); }
    /* what a feed schedule could do about it: a dwell factor per sample towards a uniform removal -- the factors' range, the
       residual before and after, the time factor (ppp_get_path_dwell) */
    void get_path_dwell() { planner.print_path_dwell(deviation_target.empty() ? nullptr : &deviation_target); }
    /* a timed feed schedule for the WayPointsList (needs getPath()): the dwell factor, the feed under a cap and an acceleration
       limit and the time per waypoint -- the waypoints by what limits them, the feed's range, the duration; writes
       <pathFile>.feed: pathFile's columns, then t and feed (ppp_get_path_feed, ppp_write_feed_file) */
    void get_path_feed() { planner.print_path_feed((std::string(planner.path_file()) + ".feed").c_str(), deviation_target.empty() ? nullptr : &deviation_target); }
    /* where this planner's cloud, the scan, stands proud of the cloud of ref (the nominal part, or the scan before the process;
       both registered in one frame): the scan's points by status, the deviation's range, mean and rms, the proud points
       (ppp_get_deviation; max_dist, smooth_radius, allowance and gain from PPP_DEVIATION_MAXDIST, _SMOOTH, _ALLOWANCE, _GAIN).
       Needs no pass.  The target map is kept: get_path_dwell() and get_path_feed() after it steer the removal towards it */
    void get_deviation(const RobotPath &ref) { planner.print_deviation(ref.planner, ppp::Planner::deviation_params_env(), &deviation_target); }
    /* this planner's cloud, the scan, registered to the cloud of ref by point-to-plane ICP from the identity (ppp_register;
       max_dist, iterations and min_step from PPP_REGISTER_MAXDIST, _ITERATIONS, _MINSTEP): prints the pairs and the rms before
       and after, the steps, the locked unknowns and T, and moves the cloud by T when the loop converged (ppp_transform_cloud:
       plan again afterwards).  ICP needs a start within the basin: a fixturing error, not an unknown pose */
    void register_to(const RobotPath &ref) { planner.print_registration(ref.planner, ppp::Planner::registration_params_env()); }
    /* register_to() against the triangles of the STL file `stl` themselves (ppp_register_mesh): the exact closest
       point and the facet's own normal, no pitch; the same lines */
    void register_to_mesh(const std::string &stl) { planner.print_mesh_registration(stl, ppp::Planner::registration_params_env()); }
    /* register_to() with the trimmed loop (ppp_register_trimmed; keep from PPP_REGISTER_KEEP, 0.8 where it is not set): a line
       with the kept and the paired counts and the cut, then register_to()'s lines over the kept pairs */
    void register_trimmed_to(const RobotPath &ref) { planner.print_registration(ref.planner, ppp::Planner::trimmed_registration_params_env()); }
    /* register_to() with the robust loop (ppp_register_robust; tune from PPP_REGISTER_TUNE, sigma_min from PPP_REGISTER_SIGMA_MIN,
       4.685 and 1e-4 mm where they are not set): a line with the used / paired counts, the median and sigma, then register_to()'s */
    void register_robust_to(const RobotPath &ref) { planner.print_registration(ref.planner, ppp::Planner::robust_registration_params_env()); }
    /* register_to_mesh() with the robust loop (ppp_register_mesh_robust): the facets' exact geometry under
       register_robust_to()'s weights, tune and sigma_min from the same variables */
    void register_robust_to_mesh(const std::string &stl) { planner.print_mesh_robust_registration(stl, ppp::Planner::robust_registration_params_env()); }
    /* register_to_mesh() with the trimmed loop (ppp_register_mesh_trimmed): the facets' exact geometry under
       register_trimmed_to()'s cut, keep from PPP_REGISTER_KEEP (0.8 where it is not set); PPP_REGISTER_BORDER=reject drops the
       candidates whose closest point lies on the mesh's border: a line with the kept, the paired and the on-border counts and the cut */
    void register_trimmed_to_mesh(const std::string &stl) { planner.print_mesh_trimmed_registration(stl, ppp::Planner::mesh_trimmed_registration_params_env()); }
    void register_global_to(const RobotPath &ref) { planner.print_global_registration(ref.planner, ppp::Planner::global_registration_params_env()); }
    /* register_global_to() against the triangles of the STL file `stl` themselves (ppp_register_mesh_global): the
       mesh's area frame against the scan's point frame, the coarse chains and the fine chain on the facets; no pitch, no normal field */
    void register_global_to_mesh(const std::string &stl) { planner.print_mesh_global_registration(stl, ppp::Planner::global_registration_params_env()); }
    /* what the contact model says about the workpiece itself, before or apart from any path: the points with a contact width,
       its smallest / mean / largest half width, the points narrower than the slice step (ppp_get_contact_field) */
    void get_contact_field() { planner.print_contact_field(); }
    /* where the planned paths leave the workpiece untouched: the uncovered points as connected regions, one line per region of
       PPP_GAPS_MIN points or more with its size, extent and centre (ppp_get_regions) */
    void get_gaps() { planner.print_gaps(); }

private:
    ppp::Planner planner;
    std::vector<double> deviation_target; /* get_deviation()'s target map; empty: a uniform target */
    std::vector<Spline> Path_set;
    std::string cloud_name;
    std::vector<std::vector<float>> WayPointsList;
};

#endif
