// cvo::CvoGPU::nlm_denoise / nlm_denoise_lab over the C-ABI (cvo_nlm_denoise / cvo_nlm_denoise_lab, include/cvo_hip.h): the
// first statement of upstream's RawImage constructor, on the device.
#include <mutex>
#include <stdexcept>
#include <string>

#include "cvo/CvoGPU.hpp"

namespace cvo {

void CvoGPU::nlm_denoise(int rows, int cols, int channels, const unsigned char* src, unsigned char* dst, float h, int template_window,
                         int search_window) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_nlm_config_t cfg{h, template_window, search_window};
  const int rc = cvo_nlm_denoise(ctx, rows, cols, channels, src, &cfg, dst);
  if (rc == CVO_E_INVALID || rc == CVO_E_UNSUPPORTED) throw std::invalid_argument(std::string("cvo_nlm_denoise: ") + cvo_last_error(ctx));
  if (rc != CVO_OK) throw std::runtime_error(std::string("cvo_nlm_denoise: ") + cvo_last_error(ctx));
}

void CvoGPU::nlm_denoise_lab(int rows, int cols, const unsigned char* lab, unsigned char* dst, float h, float h_color, int template_window,
                             int search_window) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_nlm_config_t cfg{h, template_window, search_window};
  const int rc = cvo_nlm_denoise_lab(ctx, rows, cols, lab, &cfg, h_color, dst);
  if (rc == CVO_E_INVALID || rc == CVO_E_UNSUPPORTED) throw std::invalid_argument(std::string("cvo_nlm_denoise_lab: ") + cvo_last_error(ctx));
  if (rc != CVO_OK) throw std::runtime_error(std::string("cvo_nlm_denoise_lab: ") + cvo_last_error(ctx));
}

}  // namespace cvo
