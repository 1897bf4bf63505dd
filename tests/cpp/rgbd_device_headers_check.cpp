// Compiles the veneer header (cvo/CvoGPU.hpp) on its own, host compiler only, through the statements of a front end whose
// frames never leave the device: a network's C x H x W scores and the camera's planes described where they are, the
// constructor's cloud and the recipe's cloud built from them.  Compiled to an object, not linked (the definitions are in
// host/cvo_gpu.cpp).
#include <memory>

#include "cvo/CvoGPU.hpp"

int device_front_end(const cvo::CvoGPU& gpu, const void* d_bgr, const void* d_depth_f32, const float* d_scores_chw, int rows, int cols, int classes) {
  cvo_rgbd_device_frame_t f{};
  f.rows = rows;
  f.cols = cols;
  f.channels = 3;
  f.image = d_bgr;
  f.depth = d_depth_f32;
  f.depth_type = CVO_DEPTH_F32;
  f.fx = f.fy = 525.f;
  f.cx = 319.5f;
  f.cy = 239.5f;
  f.scaling_factor = 1.f;
  f.num_classes = classes;
  f.semantic = d_scores_chw;
  f.semantic_row_stride = sizeof(float) * (size_t)cols;
  f.semantic_pixel_stride = sizeof(float);
  f.semantic_class_stride = sizeof(float) * (size_t)rows * (size_t)cols;
  std::unique_ptr<cvo::CvoGPU::ResidentClouds> edges = gpu.upload_rgbd_points_device(f, cvo::CvoPointCloud::DSO_EDGES);
  std::unique_ptr<cvo::CvoGPU::ResidentClouds> frame = gpu.upload_rgbd_device(f), coarse = gpu.upload_rgbd_device(f, 0.25f, 5.f);
  return edges->num_points(0) + frame->num_points(0) + coarse->num_points(0) + (int)frame->kept(0).size();
}
