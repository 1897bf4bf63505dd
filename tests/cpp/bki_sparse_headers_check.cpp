// Compiles the mapping veneer header (mapping/bkioctomap.h) on its own, host compiler only, through the call upstream's header
// keeps commented out - insert_pointcloud, the sparse kernel - next to insert_pointcloud_csm, from a host cloud and from a
// resident one; compiled to an object, not linked (the definitions are in host/cvo_bki.cpp).
#include "mapping/bkioctomap.h"

int sparse_mapping(const cvo::CvoGPU& gpu, const cvo::CvoPointCloud& transformed_pc, const cvo::CvoGPU::ResidentClouds& resident, const float pose12[12],
                   int num_class) {
  double sf2 = 1.0;
  double ell = 0.1;
  double free_resolution = 1;
  double ds_resolution = -1;
  double max_range = -1;
  semantic_bki::SemanticBKIOctoMap map(gpu, 0.05, 1, num_class + 1, sf2, ell, 0.0f, 1.0f, 0.65, 0.9);
  semantic_bki::point3f origin(0.5f, 0.25f, 0.f);
  map.insert_pointcloud(&transformed_pc, origin, ds_resolution, free_resolution, max_range);
  map.insert_pointcloud_csm(&transformed_pc, origin, ds_resolution, free_resolution, max_range);
  map.insert_pointcloud(resident, 0, pose12, ds_resolution, free_resolution, max_range);
  cvo::CvoPointCloud cloud_out(&map, num_class);
  return cloud_out.num_points();
}
