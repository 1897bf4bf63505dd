// Compiles the mapping veneer header (mapping/bkioctomap.h) on its own, host compiler only, through the statements of a
// mapping loop that keeps every cloud on the device: a frame inserted from where it is under its solved pose, the map read
// out as a resident cloud for the next frame.  Compiled to an object, not linked (the definitions are in host/cvo_bki.cpp).
#include <memory>

#include "mapping/bkioctomap.h"

int resident_mapping(const cvo::CvoGPU& gpu, const cvo::CvoGPU::ResidentClouds& frames, const float pose12[12], int num_class) {
  semantic_bki::SemanticBKIOctoMap map_csm(gpu, 0.05f, 1, num_class + 1, 1.0f, 1.0f, 0.0f, 1.0f, 0.65f, 0.9f);
  for (int k = 0; k < frames.size(); k++) map_csm.insert_pointcloud_csm(frames, k, pose12, -1.f, 1.f, -1.f);
  std::unique_ptr<cvo::CvoGPU::ResidentClouds> map_cloud = map_csm.resident_cloud();
  return map_cloud->num_points(0);
}
