// Mirror of the reference's src/connect.cpp / src/connect1.cpp (:7-30): ./connect cloud.pcd
// reads ../config.txt (or $PPP_CONFIG), plans, writes pathFile.  Build: see examples/Makefile.
// PPP_PATH_COVERAGE=1 prints the coverage rate of the planned paths (get_coverage's two lines, path_dynamic_alg.cpp:155-160
// keeps them commented out); PPP_PATH_CONTACTS=1 prints how evenly they cover (the largest and mean contact count, the points
// two or more slices touch); PPP_PATH_REMOVAL=1 prints how much they take off and how evenly (touched points, path length, mean /
// min / max removal and cv with the Hertzian profile); PPP_PATH_DWELL=1 prints what a feed schedule could do about it (the dwell
// factors' range, the residual before and after, the time factor); PPP_PATH_FEED=1 times the list (the waypoints by what limits
// their feed, the feed's range, the duration) and writes <pathFile>.feed, pathFile's columns with t and feed; PPP_GAPS=1 prints where they leave the workpiece untouched (the uncovered points as connected
// regions, PPP_GAPS_MIN points or more each).  PPP_DEVIATION=<reference.pcd> loads the nominal (or pre-process) cloud into a second planner and prints where the
// planned cloud, the scan, stands proud of it (points by status, the deviation's range, mean and rms; PPP_DEVIATION_MAXDIST, _SMOOTH, _ALLOWANCE, _GAIN set the
// parameters); with PPP_PATH_DWELL=1 or PPP_PATH_FEED=1 the schedule steers towards that target.  PPP_REGISTER=1 beside it
// registers the scan to that reference first (point-to-plane ICP from the identity: pairs, rms before and after, steps, locked unknowns and T are printed;
// PPP_REGISTER_MAXDIST, _ITERATIONS, _MINSTEP), before the path is planned and before the deviation is taken; PPP_REGISTER_KEEP=<share below 1> beside PPP_REGISTER=1 runs the trimmed loop instead (every evaluation keeps that share of its pairs with the smallest pair distance: for a scan with a clamp, a burr or an edge the reference does not have; the kept and the paired counts and the cut are printed); PPP_REGISTER=global does so from an unknown pose (PPP_REGISTER_CANDIDATES, _STRIDE, _COARSE_MAXDIST).  PPP_REGISTER=robust weighs every pair by Tukey's biweight of its point-to-plane residual, scaled by the median absolute residual of each evaluation (no share to choose; PPP_REGISTER_TUNE, _SIGMA_MIN; the used and the paired counts, the median and sigma are printed).  Dynamic_adjustment = false in the config plans the same walk without the adjustment.
// A name that ends in .stl (any case) is a triangle mesh, the nominal part as a CAD export: its surface is sampled on the device into the cloud (PPP_MESH_PITCH, default 0.5 mm; PPP_MESH_FACING=front keeps
// the triangles that face the origin).  PPP_DEVIATION=<reference.stl> ./connect scan.pcd measures (and with PPP_REGISTER registers) the scan against the mesh; ./connect part.stl plans on the nominal itself.
// PPP_DEVIATION=<reference.stl> PPP_DEVIATION_EXACT=1 measures against the triangles themselves (ppp_get_mesh_deviation: the closest point on the nearest triangle, along that facet's normal; no pitch):
// the same block, plus the closest points by region; PPP_DEVIATION_EXACT=signed takes the signed distance instead (ppp_get_mesh_signed_deviation: the sign of the angle-weighted pseudonormal of the feature
// the closest point lies on): the topology's counts first, a warning line when the mesh is not closed, and the points by sign and flag behind the block; PPP_TRIMESH_CELL sets the grid's cell (0 = automatic; the numbers do not depend on it), PPP_TRIMESH_ORIENT=viewpoint turns every facet normal to the origin's side.
// PPP_REGISTER=mesh PPP_DEVIATION=<reference.stl> registers against the triangles themselves (ppp_register_mesh: the exact closest point, the facet's own normal; no pitch, no estimated normal):
// ppp_register's lines, and the cloud moved by T; PPP_REGISTER=1 with an STL still registers against its samples.
// PPP_REGISTER=mesh-robust PPP_DEVIATION=<part.stl> does so under the robust loop's weights (ppp_register_mesh_robust; PPP_REGISTER_TUNE, _SIGMA_MIN): for a scan that shows a
// clamp or a strip of the table within reach of the part; PPP_REGISTER=robust's lines with the facets' numbers.
// PPP_REGISTER=mesh-trimmed PPP_DEVIATION=<part.stl> does so under the trimmed loop's cut (ppp_register_mesh_trimmed; PPP_REGISTER_KEEP, default 0.8): for a scan more contaminated than
// the median bears; PPP_REGISTER_BORDER=reject also drops every pair whose closest point lies on the border of an open mesh (the scan's overhang): a line with the kept, the
// paired and the on-border counts and the cut before and after, then PPP_REGISTER_KEEP's lines with the facets' numbers.
// PPP_REGISTER=mesh-global PPP_DEVIATION=<part.stl> registers against the triangles from an unknown pose (ppp_register_mesh_global: the mesh's area frame, the
// coarse chains and the fine chain on the facets; PPP_REGISTER_CANDIDATES, _STRIDE, _COARSE_MAXDIST): PPP_REGISTER=global's lines with the facets' numbers.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include "Path_Generate_Algorithm.h"

int main(int argc, char **argv)
{
    std::string pcd;
    for (int i = 1; i < argc; ++i) {
        size_t n = strlen(argv[i]);
        if (n > 4 && strcmp(argv[i] + n - 4, ".pcd") == 0) pcd = argv[i];
        if (ppp::Planner::is_stl_name(argv[i])) pcd = argv[i]; /* the nominal as a mesh: the path is planned on its samples */
    }
    if (pcd.empty()) {
        std::cout << "./slicing_method cad_name.pcd" << std::endl;
        return (-1);
    }
    const char *cfg = std::getenv("PPP_CONFIG");
    std::string configFile = cfg ? cfg : "../config.txt";
    path_generater path_planner = {configFile, pcd};
    const char *devf = std::getenv("PPP_DEVIATION");
    std::unique_ptr<path_generater> reference;
    if (devf && devf[0]) reference.reset(new path_generater{configFile, devf});
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
    const char *exact = std::getenv("PPP_DEVIATION_EXACT");
    if (reference && exact && !std::strcmp(exact, "signed") && ppp::Planner::is_stl_name(devf)) path_planner.get_mesh_signed_deviation(devf); /* ... with the pseudonormals' sign */
    else if (reference && exact && exact[0] == '1' && ppp::Planner::is_stl_name(devf)) path_planner.get_mesh_deviation(devf); /* against the triangles */
    else if (reference) path_planner.get_deviation(*reference); /* before the schedules: they take its target */
    const char *dwl = std::getenv("PPP_PATH_DWELL");
    if (dwl && dwl[0] == '1') path_planner.get_path_dwell();
    const char *fed = std::getenv("PPP_PATH_FEED");
    if (fed && fed[0] == '1') path_planner.get_path_feed();
    const char *fld = std::getenv("PPP_CONTACT_FIELD");
    if (fld && fld[0] == '1') path_planner.get_contact_field();
    const char *gap = std::getenv("PPP_GAPS");
    if (gap && gap[0] == '1') path_planner.get_gaps();
    path_planner.show();
    return 0;
}
