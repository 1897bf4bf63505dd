// Compiles the mapping veneer header (mapping/bkioctomap.h) on its own, host compiler only, through the statements upstream's
// driver main_local_mapping.cpp makes with it; compiled to an object, not linked (the definitions are in host/cvo_bki.cpp).
#include <iostream>

#include "mapping/bkioctomap.h"

int local_mapping(const cvo::CvoPointCloud& transformed_pc, int num_class) {
  int block_depth = 1;
  double sf2 = 1.0;
  double ell = 1.0;
  float prior = 0.0f;
  float var_thresh = 1.0f;
  double free_thresh = 0.65;
  double occupied_thresh = 0.9;
  double resolution = 0.05;
  double free_resolution = 1;
  double ds_resolution = -1;
  double max_range = -1;
  semantic_bki::SemanticBKIOctoMap map_csm(resolution, block_depth, num_class + 1, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh);
  semantic_bki::point3f origin;
  origin.x() = 0.5f;
  origin.y() = 0.25f;
  origin.z() = 0.f;
  map_csm.insert_pointcloud_csm(&transformed_pc, origin, ds_resolution, free_resolution, max_range);
  cvo::CvoPointCloud cloud_out(&map_csm, num_class);
  std::cout << origin << "\n";
  return cloud_out.num_points();
}
