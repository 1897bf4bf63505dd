// What the front-end check drivers (cvo_rgbd_check, cvo_stereo_check, cvo_lidar_check, cvo_nlm_check, cvo_sgm_check, cvo_dfilter_check) share: arrays from .npy files or raw files given as
// name:rows:cols[:channels][:u16|f32], and the FNV-1a hash they print over a cloud's rows.
#pragma once
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "utils/CvoPointCloud.hpp"

namespace cvo_check {

struct Array {
  std::vector<char> bytes;
  std::vector<int> shape;
  std::string descr;  // "|u1", "<u2", "<f4"
};

inline std::vector<std::string> split(const std::string& s, char c) {
  std::vector<std::string> out(1);
  for (char ch : s) {
    if (ch == c)
      out.emplace_back();
    else
      out.back() += ch;
  }
  return out;
}

inline Array load(const std::string& arg) {
  Array a;
  const std::vector<std::string> parts = split(arg, ':');
  std::ifstream in(parts[0], std::ios::binary);
  if (!in) throw std::runtime_error("cannot open " + parts[0]);
  std::vector<char> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (parts.size() > 1) {  // raw
    for (size_t k = 1; k < parts.size(); k++) {
      if (parts[k] == "u16") a.descr = "<u2";
      else if (parts[k] == "f32") a.descr = "<f4";
      else a.shape.push_back(std::atoi(parts[k].c_str()));
    }
    if (a.descr.empty()) a.descr = "|u1";
    a.bytes = std::move(all);
    return a;
  }
  if (all.size() < 10 || std::memcmp(all.data(), "\x93NUMPY", 6) != 0) throw std::runtime_error(parts[0] + ": neither .npy nor name:rows:cols");
  const size_t hlen = (unsigned char)all[6] == 1 ? (unsigned char)all[8] | ((size_t)(unsigned char)all[9] << 8)
                                                 : (unsigned char)all[8] | ((size_t)(unsigned char)all[9] << 8) | ((size_t)(unsigned char)all[10] << 16) | ((size_t)(unsigned char)all[11] << 24);
  const size_t hoff = (unsigned char)all[6] == 1 ? 10 : 12;
  const std::string head(all.data() + hoff, hlen);
  const size_t d = head.find("'descr'"), s = head.find("'shape'");
  if (d == std::string::npos || s == std::string::npos || head.find("'fortran_order': False") == std::string::npos) throw std::runtime_error(parts[0] + ": unsupported .npy header");
  const size_t q0 = head.find('\'', d + 7), q1 = head.find('\'', q0 + 1);
  a.descr = head.substr(q0 + 1, q1 - q0 - 1);
  const size_t p0 = head.find('(', s), p1 = head.find(')', p0);
  for (const std::string& t : split(head.substr(p0 + 1, p1 - p0 - 1), ','))
    if (t.find_first_of("0123456789") != std::string::npos) a.shape.push_back(std::atoi(t.c_str()));
  a.bytes.assign(all.begin() + (long)(hoff + hlen), all.end());
  return a;
}

inline unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

// FNV-1a over the bytes of xyz, features and geometric types, point by point
inline unsigned long long rows_hash(const cvo::CvoPointCloud& pc) {
  unsigned long long h = 14695981039346656037ull;
  for (int i = 0; i < pc.num_points(); i++) {
    h = fnv(h, pc.positions()[(size_t)i].v, 12);
    for (int c = 0; c < pc.num_features(); c++) {
      const float f = pc.features()(i, c);
      h = fnv(h, &f, 4);
    }
    h = fnv(h, &pc.geometric_types()[2 * (size_t)i], 8);
  }
  return h;
}

}  // namespace cvo_check
