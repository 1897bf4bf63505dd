// The PCL-typed LiDAR entry points of include/UnifiedCvo/pcl_interop.hpp, instantiated with the mock pcl::PointCloud of
// tests/mock_include and a point type laid out like pcl::PointXYZI, on the host: reads "n" then n rows "x y z intensity"
// from the file given, builds the cloud through a shared pointer as upstream's drivers do and prints its size and the
// first feature of its last point.
#include <cstdio>
#include <fstream>
#include <memory>

#include "pcl_interop.hpp"

#ifndef UNIFIEDCVO_HAS_PCL
#error "the mock pcl/point_cloud.h was not found: pcl_interop.hpp compiled to nothing"
#endif

struct PointXYZI {
  float x, y, z, pad, intensity, pad2[3];
};

int main(int argc, char* argv[]) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  size_t n = 0;
  in >> n;
  std::shared_ptr<pcl::PointCloud<PointXYZI>> pc(new pcl::PointCloud<PointXYZI>);
  pc->points.resize(n);
  for (PointXYZI& p : pc->points) in >> p.x >> p.y >> p.z >> p.intensity;
  cvo_lidar_rand_t rand;
  cvo_lidar_rand_seed(&rand, 1);
  const cvo::CvoPointCloud cloud = cvo::lidar_pointcloud(pc, 5000, 64, cvo::CvoPointCloud::LOAM, &rand);
  std::printf("n %d F %d last %.9g\n", cloud.num_points(), cloud.num_features(), cloud.num_points() ? cloud.features()(cloud.num_points() - 1, 0) : 0.f);
  std::vector<int> semantic(n, 2);
  cvo_lidar_rand_seed(&rand, 1);
  const cvo::CvoPointCloud labelled = cvo::lidar_pointcloud(pc, semantic, 4, 5000, 64, cvo::CvoPointCloud::LOAM, &rand);
  std::printf("n %d C %d\n", labelled.num_points(), labelled.num_classes());
  return 0;
}
