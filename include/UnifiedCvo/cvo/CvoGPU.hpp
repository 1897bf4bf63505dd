// cvo::CvoGPU for MI355X: the public API of upstream include/UnifiedCvo/cvo/CvoGPU.hpp:49-229 (pairwise
// overloads) over the C-ABI of cvo_hip.h.  Differences forced by the missing dependencies: Mat4f instead
// of Eigen::Matrix4f (same 16-float column-major layout; UnifiedCvo/eigen_interop.hpp converts where Eigen exists),
// an array of the 192-byte CvoPoint record instead of pcl::PointCloud<CvoPoint> (UnifiedCvo/pcl_interop.hpp forwards
// pcl clouds where PCL exists).  The multi-frame overload (upstream CvoGPU.hpp:101-109) runs cvo_multiframe_align.
#pragma once
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "cvo/Association.hpp"
#include "cvo/CvoFrame.hpp"
#include "cvo/CvoParams.hpp"
#include "utils/CvoPoint.hpp"
#include "utils/Calibration.hpp"
#include "utils/CvoPointCloud.hpp"
#include "utils/ImageRGBD.hpp"
#include "utils/ImageStereo.hpp"
#include "utils/data_type.hpp"

namespace cvo {

class CvoGPU {
 public:
  explicit CvoGPU(const std::string& yaml_param_file, int device = 0);
  ~CvoGPU();
  CvoGPU(const CvoGPU&) = delete;
  CvoGPU& operator=(const CvoGPU&) = delete;

  CvoParams& get_params() { return params; }
  // Upstream returns the DEVICE copy of the parameter struct (CvoGPU.hpp:52; its only users are the multi-frame IRLS
  // drivers, which hand it to CvoFrameGPU / BinaryStateGPU).  This backend passes the parameters to its kernels by
  // value at every launch, so there is no resident device copy to point at: the block the backend reads - the host
  // struct - is returned.  Valid as an opaque handle for this library's own classes; not dereferenceable in user
  // device code.
  const CvoParams* get_params_gpu() const { return &params; }
  // Upstream re-uploads *p_cpu to the device copy only (CvoGPU.cu:73-77); here the backend reads the
  // host struct at every call, so this stores *p_cpu as the parameters the next calls use.
  void write_params(const CvoParams* p_cpu);

  // 0 = success, -1 = the flow vanished (CvoGPU.cu:1454-1458).  Empty input: returns 0 and leaves
  // `transform` untouched (CvoGPU.cu:1614-1617).  Backend failures throw std::runtime_error.
  int align(const CvoPointCloud& source_points, const CvoPointCloud& target_points,
            const Mat4f& T_target_frame_to_source_frame, Mat4f& transform, Association* association = nullptr,
            double* registration_seconds = nullptr) const;
  // pcl overload (upstream CvoGPU.hpp:91-99): n records of the 192-byte AoS CvoPoint (PointSegmentedDistribution<5,19>).
  int align(const CvoPoint* source_cvo_points, int n_source, const CvoPoint* target_cvo_points, int n_target,
            const Mat4f& T_target_frame_to_source_frame, Mat4f& transform, Association* association = nullptr,
            double* registration_seconds = nullptr) const;

  // Multi-frame registration (upstream CvoGPU.cu:1637-1683 = CvoBatchIRLS::solve, IRLS.cpp:77-215, with a
  // Levenberg-Marquardt solve in place of Ceres; include/cvo_hip.h cvo_multiframe_align).  Writes every
  // frame->pose_vec and refreshes a CvoFrameGPU's transformed cloud; frames_to_hold_const[k] pins frames[k].  Every
  // frame of an edge must be in `frames`.  Frames that are all CvoFrameGPU of one device are solved from their
  // resident clouds; otherwise the frames' points are uploaded for the call.  multiframe_using_cpu is ignored (the
  // device edge state is always used).  Returns 0; argument and backend failures throw (std::invalid_argument /
  // std::runtime_error).
  int align(std::vector<CvoFrame::Ptr>& frames, const std::vector<bool>& frames_to_hold_const,
            const std::list<std::pair<CvoFrame::Ptr, CvoFrame::Ptr>>& edges, double* registration_seconds) const;

  // New: independent frame pairs solved concurrently on this object's GPU.  Returns per-pair 0 / -1.
  std::vector<int> align_batch(const std::vector<const CvoPointCloud*>& sources,
                               const std::vector<const CvoPointCloud*>& targets, const std::vector<Mat4f>& inits,
                               std::vector<Mat4f>& transforms, double* seconds = nullptr) const;
  // New: clouds that stay on the device across calls.  Upstream converts and uploads both clouds inside every align()
  // (CvoPointCloud_to_gpu, CvoGPU_impl.cu:206-285); a frame pipeline that matches a frame against several partners, or
  // a host that prepares batch k + 1 while batch k is being solved, uploads once (in parallel, cvo_cloud_upload_many).
  class ResidentClouds {
   public:
    ~ResidentClouds();
    ResidentClouds(const ResidentClouds&) = delete;
    ResidentClouds& operator=(const ResidentClouds&) = delete;
    int size() const { return (int)handles.size(); }
    int num_points(int k) const { return cvo_cloud_size(handles[(size_t)k]); }
    // upload_clouds_voxel: the indices of cloud k's points that were kept, ascending (empty after upload_clouds)
    const std::vector<int>& kept(int k) const { return kept_[(size_t)k]; }

   private:
    friend class CvoGPU;
    ResidentClouds() = default;
    std::vector<cvo_cloud*> handles;
    std::vector<std::vector<int>> kept_;
  };
  std::unique_ptr<ResidentClouds> upload_clouds(const std::vector<const CvoPointCloud*>& clouds, int host_threads = 0) const;
  std::vector<int> align_batch(const ResidentClouds& sources, const ResidentClouds& targets, const std::vector<Mat4f>& inits,
                               std::vector<Mat4f>& transforms, double* seconds = nullptr) const;
  // New: a resident cloud from rows that are ALREADY in this object's device memory (cvo_cloud_from_device /
  // _aos192, include/cvo_hip.h: strided arrays or 192-byte CvoPoint records, complete when the call is made) - what
  // upload_clouds returns for one cloud, without a host copy.  Refusals (host pointers, strides, row indices) throw.
  std::unique_ptr<ResidentClouds> upload_device(const cvo_device_rows_t& rows) const;
  std::unique_ptr<ResidentClouds> upload_device_aos192(const CvoPoint* d_pts, int n) const;
  // New: a resident cloud from an RGB-D FRAME that is already in this object's device memory (cvo_cloud_from_rgbd_device /
  // _recipe, include/cvo_hip.h: dense image / gray / depth planes, class scores with byte strides, complete when the call
  // is made).  upload_rgbd_points_device: CvoPointCloud(ImageRGBD, Calibration, method) for DSO_EDGES / FULL as
  // upload_clouds would hold it; upload_rgbd_device: the multi-frame drivers' recipe (leaf <= 0 takes
  // params.multiframe_downsample_voxel_size) - edge points first.  kept(0): the pixel index v * cols + u of every point.
  // No plane and no row crosses to the host.  Refusals (host pointers, strides, extents, other methods) throw.
  std::unique_ptr<ResidentClouds> upload_rgbd_points_device(const cvo_rgbd_device_frame_t& frame, CvoPointCloud::PointSelectionMethod method) const;
  std::unique_ptr<ResidentClouds> upload_rgbd_device(const cvo_rgbd_device_frame_t& frame, float leaf = 0.f, float edge_divisor = 4.f) const;
  // New: what the multi-frame drivers do right after the solve (merge_transformed_pc + a VoxelMap of side leaf / 2,
  // main_covisMap_test.cpp:183-215, 464-534) without a host copy of any frame (cvo_cloud_merge, include/cvo_hip.h): ONE
  // resident cloud (size() == 1) of the rows of every cloud of `clouds`, in original order, cloud after cloud, each moved by
  // its pose - poses: 12 doubles per cloud, 3x4 row-major, what the ResidentClouds align() leaves; nullptr: nothing is moved
  // - and thinned to the lowest row of every voxel.  voxel_size == 0: the concatenation; < 0:
  // params.multiframe_downsample_voxel_size / 2, the covis driver's value.  kept(0): the global rows of the result's points.
  // download: cloud k's rows in original order, bit for bit what was uploaded (cvo_cloud_download); attributes the cloud
  // does not hold are left out (F = 0 / no classes / types 0).  Refusals throw.
  std::unique_ptr<ResidentClouds> merge(const ResidentClouds& clouds, const std::vector<double>* poses, float voxel_size = 0.f) const;
  CvoPointCloud download(const ResidentClouds& clouds, int k) const;
  // New: keyframe depth filtering, the last loops of main_depth_filtering.cpp (208-298), without a host copy of any
  // association or frame (cvo_depth_filter, include/cvo_hip.h): cloud kf_index of `kf` refined from every cloud of `frames`
  // - T_t2s[k] is the association's transform for frame k (the driver's T_t^-1 T_s), T_s2t[k] the one whose third row gives
  // an associated point's depth in the keyframe's frame (the driver's T_s^-1 T_t), `kernel` the non-isotropic kernel - as ONE
  // resident cloud (size() == 1): the rows with more than min_count observations, moved along their rays.  kept(0): their
  // original indices.  The CvoPointCloud overload mirrors the driver's last loop: clouds in, kf_filtered out.  Refusals throw.
  std::unique_ptr<ResidentClouds> depth_filter(const ResidentClouds& kf, int kf_index, const ResidentClouds& frames,
                                               const std::vector<Mat4f>& T_t2s, const std::vector<Mat4f>& T_s2t, const Mat3f& kernel,
                                               int min_count = 3) const;
  CvoPointCloud depth_filter(const CvoPointCloud& kf, const std::vector<const CvoPointCloud*>& frames, const std::vector<Mat4f>& T_t2s,
                             const std::vector<Mat4f>& T_s2t, const Mat3f& kernel, int min_count = 3) const;
  // New: voxel-grid downsampling on the device - what the drivers do with cvo::VoxelMap before align()
  // (main_multi_frame_irls_tum.cpp:290-335; utils/VoxelMap.hpp is the host class): of every occupied voxel of side
  // voxel_size the point with the LOWEST index is kept, in ascending index (cvo_voxel_select, include/cvo_hip.h).
  // voxel_size <= 0 takes params.multiframe_downsample_voxel_size.  voxel_downsample returns the kept points as a host
  // cloud (*kept: their indices); upload_clouds_voxel leaves them resident, attributes gathered on the host for the
  // survivors only (a loop over cvo_cloud_upload_voxel).  Refusals (non-finite coordinates, |k| >= 2^20) throw.
  CvoPointCloud voxel_downsample(const CvoPointCloud& cloud, float voxel_size = 0.f, std::vector<int>* kept = nullptr) const;
  std::unique_ptr<ResidentClouds> upload_clouds_voxel(const std::vector<const CvoPointCloud*>& clouds, float voxel_size = 0.f) const;
  // New: the RGB-D front end on the device (cvo_rgbd_points / cvo_cloud_upload_rgbd, include/cvo_hip.h).  rgbd_points is
  // CvoPointCloud(raw_image, calib, method) with the selector and the depth test run by the kernels.  upload_rgbd is the
  // multi-frame RGB-D drivers' per-frame block (main_multi_frame_irls_tum.cpp:279-335) in one call: FULL and DSO_EDGES
  // candidates, voxel grids of side leaf (surface) and leaf / edge_divisor (edge; 4 TUM, 5 Tartan / KITTI, 10 covis), the
  // survivors as colour points of type EDGE / SURFACE, edge first, resident (size() == 1).  leaf <= 0 takes
  // params.multiframe_downsample_voxel_size.  pixel / is_edge (optional): v * cols + u and the set of every point.
  // Defined in host/cvo_rgbd.cpp for DepthType uint16_t / float.
  template <typename DepthType>
  CvoPointCloud rgbd_points(const ImageRGBD<DepthType>& raw_image, const Calibration& calib, CvoPointCloud::PointSelectionMethod method,
                            std::vector<int>* pixel = nullptr) const;
  template <typename DepthType>
  std::unique_ptr<ResidentClouds> upload_rgbd(const ImageRGBD<DepthType>& raw_image, const Calibration& calib, float leaf = 0.f,
                                              float edge_divisor = 4.f, std::vector<int>* pixel = nullptr,
                                              std::vector<unsigned char>* is_edge = nullptr) const;
  // New: the stereo front end on the device (cvo_stereo_points / cvo_cloud_upload_stereo / _recipe, include/cvo_hip.h), from
  // the frame's own disparity.  stereo_points is CvoPointCloud(raw_image, calib, method) with the selector, the keep predicate
  // and the back-projection run by the kernels.  upload_stereo is the pairwise KITTI driver's cloud
  // (main_cvo_gpu_align_raw_image.cpp:61-91), resident (size() == 1).  upload_stereo_recipe is the multi-frame KITTI driver's
  // per-frame block (main_multi_frame_irls_kitti.cpp:235-292): upload_rgbd's recipe on the stereo points, divisor 5.
  // Defined in host/cvo_stereo.cpp.
  CvoPointCloud stereo_points(const ImageStereo& raw_image, const Calibration& calib,
                              CvoPointCloud::PointSelectionMethod method = CvoPointCloud::CV_FAST, std::vector<int>* pixel = nullptr) const;
  std::unique_ptr<ResidentClouds> upload_stereo(const ImageStereo& raw_image, const Calibration& calib,
                                                CvoPointCloud::PointSelectionMethod method = CvoPointCloud::CV_FAST,
                                                std::vector<int>* pixel = nullptr) const;
  std::unique_ptr<ResidentClouds> upload_stereo_recipe(const ImageStereo& raw_image, const Calibration& calib, float leaf = 0.f,
                                                       float edge_divisor = 5.f, std::vector<int>* pixel = nullptr,
                                                       std::vector<unsigned char>* is_edge = nullptr) const;
  // New: the LiDAR front end on the device (cvo_cloud_upload_lidar, include/cvo_hip.h): the cloud of
  // CvoPointCloud(xyzi, n, [semantic, num_classes,] target, beam_num) - LOAM selection with the HDL-64 configuration -
  // selected by the kernels, resident (size() == 1).  semantic: nullptr or n class ids.  rand as in the constructors.
  // Defined in host/cvo_lidar.cpp.
  std::unique_ptr<ResidentClouds> upload_lidar(const float* xyzi, int n, const std::vector<int>* semantic, int num_classes, int beam_num,
                                               std::vector<int>* index = nullptr, cvo_lidar_rand_t* rand = nullptr) const;
  // New: the first statement of upstream's RawImage constructor on the device (cvo_nlm_denoise / cvo_nlm_denoise_lab,
  // include/cvo_hip.h): cv::fastNlMeansDenoising of an 8-bit image of 1 .. 3 interleaved channels, and the middle of
  // cv::fastNlMeansDenoisingColored on a Lab image (BGR <-> Lab stays the caller's).  dst may be src.  Refusals throw
  // std::invalid_argument.  Defined in host/cvo_nlm.cpp.
  // New: the library's own stereo matcher on the device (cvo_stereo_disparity, include/cvo_hip.h): the float left disparity
  // of a rectified pair of rows x cols gray planes, invalid = -10, by semi-global matching over a census cost - NOT upstream's
  // libelas.  config == nullptr: cvo_sgm_config_default.  dfilter given: cvo_stereo_disparity_filtered - the matcher, then
  // disparity_filter of its map, which stays on the device in between.  Refusals throw std::invalid_argument.  Defined in
  // host/cvo_sgm.cpp.
  std::vector<float> stereo_disparity(int rows, int cols, const unsigned char* left, const unsigned char* right,
                                      const cvo_sgm_config_t* config = nullptr, const cvo_dfilter_config_t* dfilter = nullptr) const;
  // New: libelas's three disparity post-passes on the device (cvo_disparity_filter, include/cvo_hip.h): removeSmallSegments,
  // gapInterpolation and adaptiveMean of a rows x cols float map whose invalid pixels are negative (they leave as -10), the
  // matcher's or any other's.  config == nullptr: cvo_dfilter_config_default (libelas's ROBOTICS setting).  Refusals throw
  // std::invalid_argument.  Defined in host/cvo_sgm.cpp.
  std::vector<float> disparity_filter(int rows, int cols, const float* disparity, const cvo_dfilter_config_t* config = nullptr) const;
  void nlm_denoise(int rows, int cols, int channels, const unsigned char* src, unsigned char* dst, float h = 10.f, int template_window = 7,
                   int search_window = 21) const;
  void nlm_denoise_lab(int rows, int cols, const unsigned char* lab, unsigned char* dst, float h = 10.f, float h_color = 10.f,
                       int template_window = 7, int search_window = 21) const;
  // New: multi-frame registration over resident clouds (cvo_multiframe_align as it is): poses 12 doubles per cloud (3x4
  // row-major, updated in place), edges pairs of indices into `clouds`.
  int align(const ResidentClouds& clouds, std::vector<double>& poses, const std::vector<bool>& frames_to_hold_const,
            const std::vector<std::pair<int, int>>& edges, double* registration_seconds = nullptr) const;
  // New: a STREAM of resident pairs through `slots` in-flight slots (cvo_batch_open / _submit / _poll, include/cvo_hip.h):
  // a pair that finishes hands its slice of the workspace to the next one at the next chunk boundary, so the GPU stays
  // full however different the pairs' iteration counts are - upstream's own use is a frame stream with warm starts
  // (main_cvo_gpu_align_raw_image.cpp:100-170).  pairs[k] = {index into sources, index into targets}; max_iterations[k]
  // (optional) = that pair's own iteration limit.  Transforms / return values in submission order, every pose
  // bit-identical to a solo align().  Memory: the workspace is sized up front for min(slots, pairs) pairs of the LARGEST
  // source x target sizes of the call - ~139 MB per slot at 10k x 10k with nearest_neighbors_max = 512 (17 GB for the
  // default 128 slots), N * M / 8 bytes of candidate bitmap per slot beyond that; a request that does not fit fails with
  // a sized CVO_E_NOMEM message (cvo_last_error).  The queue is closed on every way out, exceptions included.
  std::vector<int> align_stream(const ResidentClouds& sources, const ResidentClouds& targets,
                                const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& inits,
                                std::vector<Mat4f>& transforms, int slots = 128, const std::vector<int>* max_iterations = nullptr,
                                double* seconds = nullptr) const;
  // New: many scores in one call (cvo_inner_product_batch / cvo_function_angle_batch, include/cvo_hip.h).  Job k scores
  // sources[pairs[k].first] against targets[pairs[k].second] under T[k] with lengthscale ell[k] (ell may also hold ONE
  // value for every job); every value is bit-identical to inner_product_gpu / function_angle of the same clouds.
  std::vector<float> inner_product_batch(const ResidentClouds& sources, const ResidentClouds& targets,
                                         const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& T,
                                         const std::vector<float>& ell) const;
  std::vector<float> function_angle_batch(const ResidentClouds& sources, const ResidentClouds& targets,
                                          const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& T,
                                          const std::vector<float>& ell, bool is_approximate = true) const;
  // cvo_ctx_advice of this object's context ("" = nothing to report; see include/cvo_hip.h, hardware queues)
  std::string advice() const;

  float function_angle(const CvoPointCloud& source_points, const CvoPointCloud& target_points,
                       const Mat4f& T_target_frame_to_source_frame, float ell, bool is_approximate = true,
                       bool is_gpu = true) const;
  float inner_product_gpu(const CvoPointCloud& source_points, const CvoPointCloud& target_points,
                          const Mat4f& T_target_frame_to_source_frame, float ell) const;
  // pcl overloads (upstream CvoGPU.hpp:167-171, 220-224; CvoGPU.cu:1796-1809, 1848-1873)
  float function_angle(const CvoPoint* source_cvo_points, int n_source, const CvoPoint* target_cvo_points, int n_target,
                       const Mat4f& T_target_frame_to_source_frame, float ell, bool is_approximate = true) const;
  float inner_product_gpu(const CvoPoint* source_cvo_points, int n_source, const CvoPoint* target_cvo_points, int n_target,
                          const Mat4f& T_target_frame_to_source_frame, float ell) const;
  // The reference's HOST function of the same name (upstream CvoGPU.cpp:95-213): NOT the function the GPU path
  // computes - plain ell (no range factor), no neighbour cap, no colour / semantic cut-offs, radius search instead of
  // the ordered scan - and not a fallback for anything: function_angle(..., is_gpu = false) routes here as upstream's does.
  float inner_product_cpu(const CvoPointCloud& source_points, const CvoPointCloud& target_points,
                          const Mat4f& T_target_frame_to_source_frame, float ell) const;
  void compute_association_gpu(const CvoPointCloud& source_points, const CvoPointCloud& target_points,
                               const Mat4f& T_target_frame_to_source_frame, float lengthscale,
                               Association& association) const;
  // Non-isotropic (Mahalanobis) kernel d^T K^-1 d: no geometric cut-off, geometric types off (CvoGPU.cu:1967-1988).
  void compute_association_gpu(const CvoPointCloud& source_points, const CvoPointCloud& target_points,
                               const Mat4f& T_target_frame_to_source_frame, const Mat3f& non_isotropic_kernel,
                               Association& association) const;
  // New: a semantic voxel map on this object's context (cvo_map_open, include/cvo_hip.h; mapping/bkioctomap.h wraps it in upstream's
  // names).  The caller closes it with cvo_map_close before this object goes.  Refusals throw std::invalid_argument.  last_error:
  // cvo_last_error of the context.  Defined in host/cvo_bki.cpp.
  cvo_map* map_open(const cvo_map_config_t& cfg, long long initial_voxels = 0) const;
  // New: the map's two calls that keep every cloud on the device (cvo_map_insert_cloud / cvo_map_cloud_resident; SemanticBKIOctoMap's
  // insert_pointcloud_csm(const ResidentClouds&, ...) and resident_cloud() are these): cloud k of `clouds` as the hits of one insert,
  // moved by pose12 (nullptr: as stored) and seen from origin (nullptr: the pose's translation); the occupied voxels as one
  // resident cloud.  Refusals throw std::invalid_argument.
  void map_insert_cloud(cvo_map* map, const ResidentClouds& clouds, int k, const float* pose12, const float* origin) const;
  std::unique_ptr<ResidentClouds> map_resident_cloud(cvo_map* map) const;
  // New: cvo_map_query_cloud for cloud k of `clouds` (SemanticBKIOctoMap::search(const ResidentClouds&, ...) is this): what is at
  // its rows, moved by pose12 (nullptr: as stored), without a host copy.  Refusals throw std::invalid_argument.
  void map_query_cloud(cvo_map* map, const ResidentClouds& clouds, int k, const float* pose12, const cvo_map_query_out_t& out) const;
  std::string last_error() const;

 private:
  CvoParams params;
  cvo_ctx* ctx = nullptr;
  // Upstream's align() const is re-entrant (all state is per call, CvoGPU.cu:1605-1632); here the const entry points
  // share one context (streams, cached workspace, graphs), which is not thread-safe: they serialise on this mutex, so
  // concurrent callers of ONE object get upstream's behaviour (upstream serialises them on the default stream as
  // well).  For concurrency use one CvoGPU per host thread, or align_batch.
  mutable std::mutex call_mutex;
  std::vector<float> score_batch(const ResidentClouds& sources, const ResidentClouds& targets,
                                 const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& T,
                                 const std::vector<float>& ell, int function_angle) const;
};

}  // namespace cvo
