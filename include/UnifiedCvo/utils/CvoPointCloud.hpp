// Host point-cloud container: the accessor subset of upstream utils/CvoPointCloud.hpp:126-188 that the
// align() path and its drivers use, the RGB-D image constructor (FULL / DSO_EDGES) and the stereo image constructor from a
// given disparity (CV_FAST / DSO_EDGES / FULL) and the LiDAR constructors (LOAM) over plain arrays.
#pragma once
#include <string>
#include <vector>

#include "utils/data_type.hpp"

#ifndef FEATURE_DIMENSIONS
#define FEATURE_DIMENSIONS 5
#endif
#ifndef NUM_CLASSES
#define NUM_CLASSES 19
#endif

namespace cvo {

class Calibration;
template <typename DepthType>
class ImageRGBD;
class ImageStereo;
}  // namespace cvo
struct cvo_lidar_rand_t;
namespace semantic_bki {
class SemanticBKIOctoMap;
}
namespace cvo {

class CvoPointCloud {
 public:
  enum GeometryType { EDGE = 0, SURFACE = 1 };
  // upstream CvoPointCloud.hpp:39-49, same names and values
  enum PointSelectionMethod { CV_FAST, RANDOM, DSO_EDGES, DSO_EDGES_WITH_RANDOM, LIDAR_EDGES, CANNY_EDGES, EDGES_ONLY, LOAM, FULL };

  CvoPointCloud();
  CvoPointCloud(int feature_dimensions, int num_classes);
  // A file on disk.  A text file in upstream's own format (CvoPointCloud.cpp:89-148: "N F C" then per point
  // "x y z f_1..f_F l_1..l_C", points farther than 55 m dropped) is read as upstream's string constructor does.
  // A file that starts with a PCD header is read as the drivers do with pcl::io::loadPCDFile + the pcl::PointXYZ /
  // PointXYZRGB / PointXYZI constructors (CvoPointCloud.cpp:569-594, 633-652): ASCII, FIELDS "x y z", "x y z rgb"
  // or "x y z intensity" (one feature: the cvo_gpu_lidar_lib flavour, FEATURE_DIMENSIONS = 1).
  explicit CvoPointCloud(const std::string& filename);
  // upstream CvoPointCloud.cpp:1157-1199: "N F C" then per point "u v idepth f_1..f_F x y z l_1..l_C"; 0 / -1
  int read_cvo_pointcloud_from_file(const std::string& filename);

  // upstream CvoPointCloud.cpp:459-553 for DepthType uint16_t / float (utils/ImageRGBD.hpp, utils/Calibration.hpp) and
  // pt_selection_method FULL or DSO_EDGES, on the host (cvo_rgbd_points_host, include/cvo_hip.h, states the contract: F =
  // channels + 2, point order, the gradient-index quirk); every other method throws std::invalid_argument (OpenCV
  // detectors and rand() are not restated).  The image is taken as it is: denoise it first with CvoGPU::nlm_denoise(_lab) (utils/RawImage.hpp).
  // pixel (optional): v * cols + u of every point.  Defined in host/cvo_rgbd.cpp.
  template <typename DepthType>
  CvoPointCloud(const ImageRGBD<DepthType>& raw_image, const Calibration& calib, PointSelectionMethod pt_selection_method,
                std::vector<int>* pixel = nullptr);

  // upstream CvoPointCloud.cpp:680-773 (utils/ImageStereo.hpp: the disparity is the caller's, libelas is not part of this
  // library) for pt_selection_method CV_FAST (upstream's default), DSO_EDGES or FULL, on the host (cvo_stereo_points_host,
  // include/cvo_hip.h, states the contract: the keep predicate, the float arithmetic, F = channels + 2); every other method
  // throws std::invalid_argument.  pixel (optional): v * cols + u of every point.  Defined in host/cvo_stereo.cpp.
  CvoPointCloud(const ImageStereo& raw_image, const Calibration& calib, PointSelectionMethod pt_selection_method = CV_FAST,
                std::vector<int>* pixel = nullptr);

  // upstream CvoPointCloud.cpp:964-1038 and :1040-1136 (pcl::PointCloud<pcl::PointXYZI>::Ptr; the PCL-typed overloads are
  // in pcl_interop.hpp) for pt_selection_method LOAM, the default, on the host (cvo_lidar_select_host, include/cvo_hip.h:
  // edge_detection, then LeGO-LOAM's selection with the HDL-64 configuration and beam_num): xyzi is n x 4 floats - x, y, z,
  // intensity in upstream's axes, in scan order; F = 1 (intensity), type (1, 0), one-hot labels with `semantic` (n class ids,
  // -1 = unlabelled).  target_num_points is accepted and unused, as upstream leaves it.  RANDOM and LIDAR_EDGES throw
  // std::invalid_argument.  rand: the stream the thinning draws from (cvo_lidar_rand_seed); nullptr = one stream per
  // process that starts as an unseeded std::rand() does, as upstream draws.  index (optional): the point of every row.
  // Defined in host/cvo_lidar.cpp.
  CvoPointCloud(const float* xyzi, int n, int target_num_points, int beam_num, PointSelectionMethod pt_selection_method = LOAM,
                std::vector<int>* index = nullptr, cvo_lidar_rand_t* rand = nullptr);
  CvoPointCloud(const float* xyzi, int n, const std::vector<int>& semantic, int num_classes, int target_num_points, int beam_num,
                PointSelectionMethod pt_selection_method = LOAM, std::vector<int>* index = nullptr, cvo_lidar_rand_t* rand = nullptr);

  // upstream bkioctomap.cpp:22-78 (mapping/bkioctomap.h): the OCCUPIED voxels of a semantic voxel map - centre, fs / sum(ms[1:]),
  // ms[1..] / sum(ms) -, here in ascending key order (cvo_map_cloud, include/cvo_hip.h); F = 5.  num_classes must be the map's;
  // std::invalid_argument otherwise.  Defined in host/cvo_bki.cpp.
  CvoPointCloud(const semantic_bki::SemanticBKIOctoMap* map, const int num_classes);

  static CvoPointCloud from_xyz(const float* xyz, int n);                                // type (1,0), F = 0
  static CvoPointCloud from_xyzrgb(const float* xyz, const unsigned char* rgb, int n);   // type (0,1), F = 5

  // New: the cloud of the rows `indices`, in that order (what a voxel selection keeps: CvoGPU::voxel_downsample).
  // Throws std::out_of_range on an index outside the cloud.
  CvoPointCloud select(const std::vector<int>& indices) const;

  static void transform(const Mat4f& pose, const CvoPointCloud& input, CvoPointCloud& output);
  friend CvoPointCloud operator+(CvoPointCloud a, const CvoPointCloud& b);

  int num_points() const { return num_points_; }
  int size() const { return num_points_; }
  int num_classes() const { return num_classes_; }
  int num_features() const { return feature_dimensions_; }
  int feature_dimensions() const { return feature_dimensions_; }
  const std::vector<Vec3f>& positions() const { return positions_; }
  Vec3f at(unsigned int index) const { return positions_[index]; }
  const MatXf& labels() const { return labels_; }
  // upstream CvoPointCloud.hpp:141-143 (CvoPointCloud.cpp:1282-1286): one point's class distribution / feature row /
  // (edge, surface) pair by value
  VecXf label_at(unsigned int index) const { return labels_.row((int)index); }
  VecXf feature_at(unsigned int index) const { return features_.row((int)index); }
  Vec2f geometry_type_at(unsigned int index) const {
    return Vec2f{{geometric_types_[(size_t)index * 2], geometric_types_[(size_t)index * 2 + 1]}};
  }
  const MatXf& semantics() const { return labels_; }
  const MatXf& features() const { return features_; }
  const std::vector<float>& geometric_types() const { return geometric_types_; }

  void reserve(int num_points, int feature_dims, int num_classes);
  // returns -1 if the cloud was not reserved, the index is out of range or geometric_type.size() != 2
  int add_point(int index, const Vec3f& xyz, const std::vector<float>& feature, const std::vector<float>& label,
                const std::vector<float>& geometric_type);

  // upstream CvoPointCloud.cpp:1289-1362; PCD files in the layout of pcl::io::savePCDFileASCII (PCL 1.9.1)
  void write_to_color_pcd(const std::string& name) const;      // PointXYZRGB: r,g,b <- features 2,1,0 as upstream
  void write_to_pcd(const std::string& name) const;            // PointXYZ
  void write_to_label_pcd(const std::string& name) const;      // PointXYZL: argmax label (nothing if no classes)
  void write_to_intensity_pcd(const std::string& name) const;  // PointXYZI: first feature
  void write_to_txt(const std::string& name) const;            // "N C" header, then xyz line + features/labels line

 private:
  int num_points_ = 0;
  int num_classes_ = 0;
  int feature_dimensions_ = 0;
  std::vector<Vec3f> positions_;
  MatXf features_;
  MatXf labels_;
  std::vector<float> geometric_types_;
};

}  // namespace cvo
