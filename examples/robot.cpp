// A caller of the RobotPath drop-in (include/robot_path.h): ./robot cloud.pcd [radius].  The reference declares the class
// (robot_path.h:58-98) but nothing constructs it -- the header does not compile upstream -- so this is the shape of
// src/connect.cpp with the three-argument constructor.  PPP_PATH_COVERAGE=1 prints the coverage rate of the planned paths,
// PPP_PATH_CONTACTS=1 their contact counts, PPP_PATH_REMOVAL=1 the predicted removal, PPP_PATH_DWELL=1 a dwell schedule
// towards a uniform removal, PPP_PATH_FEED=1 the timed feed schedule of the list (written to <pathFile>.feed), PPP_GAPS=1 the regions they leave uncovered,
// PPP_DEVIATION=<reference.pcd> the deviation of the cloud against that reference (its target goes to PPP_PATH_DWELL / PPP_PATH_FEED);
// PPP_REGISTER=1 beside it registers the cloud to that reference first, before the path is planned (pairs, rms before and after, steps, locked unknowns, T); PPP_REGISTER_KEEP=<share below 1> beside PPP_REGISTER=1 runs the trimmed loop instead (every evaluation keeps that share of its pairs with the smallest pair distance: for a scan with a clamp, a burr or an edge the reference does not have; the kept and the paired counts and the cut are printed); PPP_REGISTER=global does so from an unknown pose.  PPP_REGISTER=robust weighs every pair by Tukey's biweight of its point-to-plane residual, scaled by the median absolute residual of each evaluation (no share to choose; PPP_REGISTER_TUNE, _SIGMA_MIN).
// PPP_REGISTER=mesh PPP_DEVIATION=<reference.stl> registers against the triangles themselves (ppp_register_mesh: the exact closest point, the facet's own normal; no pitch, no estimated normal):
// ppp_register's lines, and the cloud moved by T; PPP_REGISTER=1 with an STL still registers against its samples.
// PPP_REGISTER=mesh-robust PPP_DEVIATION=<part.stl> does so under the robust loop's weights (ppp_register_mesh_robust; PPP_REGISTER_TUNE, _SIGMA_MIN): for a scan that shows a
// clamp or a strip of the table within reach of the part; PPP_REGISTER=robust's lines with the facets' numbers.
// PPP_REGISTER=mesh-trimmed PPP_DEVIATION=<part.stl> does so under the trimmed loop's cut (ppp_register_mesh_trimmed; PPP_REGISTER_KEEP, default 0.8): for a scan more contaminated than
// the median bears; PPP_REGISTER_BORDER=reject also drops every pair whose closest point lies on the border of an open mesh (the scan's overhang): a line with the kept, the
// paired and the on-border counts and the cut before and after, then PPP_REGISTER_KEEP's lines with the facets' numbers.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include "ppp_planner.hpp"
#include "robot_path.h"

int main(int argc, char **argv)
{
    std::string pcd;
    double radius = 6;
    for (int i = 1; i < argc; ++i) {
        size_t n = strlen(argv[i]);
        if (n > 4 && strcmp(argv[i] + n - 4, ".pcd") == 0) pcd = argv[i];
        else radius = atof(argv[i]);
    }
    if (pcd.empty()) {
        std::cout << "./robot cad_name.pcd [radius]" << std::endl;
        return (-1);
    }
    const char *cfg = std::getenv("PPP_CONFIG");
    std::string configFile = cfg ? cfg : "../config.txt";
    RobotPath path_planner(configFile, pcd, radius);
    const char *devf = std::getenv("PPP_DEVIATION");
    std::unique_ptr<RobotPath> reference;
    if (devf && devf[0]) reference.reset(new RobotPath(configFile, devf, radius));
    const char *reg = std::getenv("PPP_REGISTER");
    if (reference && reg && reg[0] == '1') { /* before the plan: it moves the cloud; PPP_REGISTER_KEEP=<share below 1>: the trimmed loop */
        if (ppp::Planner::trimmed_registration_asked()) path_planner.register_trimmed_to(*reference);
        else path_planner.register_to(*reference);
    }
    if (reference && reg && std::string(reg) == "global") path_planner.register_global_to(*reference); /* from an unknown pose */
    if (reference && reg && std::string(reg) == "robust") path_planner.register_robust_to(*reference); /* Tukey weights: no keep to choose */
    if (reference && reg && std::string(reg) == "mesh" && ppp::Planner::is_stl_name(devf)) path_planner.register_to_mesh(devf); /* on the facets, not on their samples */
    if (reference && reg && std::string(reg) == "mesh-robust" && ppp::Planner::is_stl_name(devf)) path_planner.register_robust_to_mesh(devf); /* the facets under Tukey weights */
    if (reference && reg && std::string(reg) == "mesh-trimmed" && ppp::Planner::is_stl_name(devf)) path_planner.register_trimmed_to_mesh(devf); /* the facets under the cut, the border rejected on request */
    if (reference && reg && std::string(reg) == "mesh-global" && ppp::Planner::is_stl_name(devf)) path_planner.register_global_to_mesh(devf); /* the facets, from an unknown pose */
    path_planner.GenPath();
    path_planner.getPath();
    const char *cov = std::getenv("PPP_PATH_COVERAGE");
    if (cov && cov[0] == '1') path_planner.get_path_coverage();
    const char *con = std::getenv("PPP_PATH_CONTACTS");
    if (con && con[0] == '1') path_planner.get_path_contacts();
    const char *rem = std::getenv("PPP_PATH_REMOVAL");
    if (rem && rem[0] == '1') path_planner.get_path_removal();
    if (reference) path_planner.get_deviation(*reference); /* before the schedules: they take its target */
    const char *dwl = std::getenv("PPP_PATH_DWELL");
    if (dwl && dwl[0] == '1') path_planner.get_path_dwell();
    const char *fed = std::getenv("PPP_PATH_FEED");
    if (fed && fed[0] == '1') path_planner.get_path_feed();
    const char *fld = std::getenv("PPP_CONTACT_FIELD");
    if (fld && fld[0] == '1') path_planner.get_contact_field();
    const char *gap = std::getenv("PPP_GAPS");
    if (gap && gap[0] == '1') path_planner.get_gaps();
    path_planner.show();
    std::cout << "waypoints: " << path_planner.waypoints().size() << std::endl;
    return 0;
}
