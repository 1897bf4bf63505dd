// Drives upstream's own compiled mapping code (bkiblock.cpp, bkioctree.cpp, bkioctree_node.cpp, point3f.cpp, rtree.h) on case
// files, so that tests/np_bki.py is held to upstream's object code and not to a reading of its text
// (scripts/make_bki_upstream_golden.py -> tests/golden/bki_upstream.npz).  Built by oracle/Makefile into oracle/_ref/.
//
//     bki_upstream CASES RESULTS
//
// Both files are sequences of little-endian 32-bit words; a float crosses as its bit pattern, a 64-bit key as (low, high).
// CASES is a list of operations, each an opcode followed by its words; RESULTS holds their answers in the same order.
//   1 keys:    resolution, n, n * (x, y, z)
//              -> per point: key, hash_key_to_block(key) (3), Block(that centre).get_loc(begin_leaf()) (3)
//   2 members: resolution, n, n * (x, y, z)
//              -> per point: m, m * key - the blocks among the 125 around the point's own key whose box query returns it
//   3 node:    num_class, prior, free_thresh, occupied_thresh, steps, steps * (ybars (num_class), fbars (5))
//              -> per step: ms, fs (5), state, semantics, get_probs, get_occupied_probs (num_class - 1), get_features (5)
//   4 insert:  resolution, num_class, prior, free_thresh, occupied_thresh, frames,
//              frames * (n, n * (x, y, z, class, has_row, row (5)))
//              -> per frame: v, v * (key, updated in this frame, ms, fs (5), state, leaf location (3), get_features (5),
//                 get_occupied_probs (num_class - 1)) over every block updated so far, ascending key
// Everything that decides a value is upstream's: the key and centre functions, the R-tree and its box test, Semantics.  Own to
// this file: the file format, the loops over candidate blocks and the class histogram (upstream's all-ones counting-sensor
// product), and the box of a block, restated from get_gp_points_in_bbox.  A candidate whose index leaves the key's 20-bit
// field cannot be written as a key and is passed over.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "mapping/bkiblock.h"
#include "mapping/rtree.h"

namespace semantic_bki {

struct Hit {
  float p[3];
  uint32_t cls, has_row;
  float row[5];
};

// The name upstream's types befriend: sets their private statics and reads a leaf's ms / fs.
class SemanticBKIOctoMap {
 public:
  static void grid(float resolution) {  // block_depth 1
    Block::resolution = resolution;
    Block::size = resolution;
    Block::key_loc_map = init_key_loc_map(resolution, 1);
    SemanticOcTree::max_depth = 1;
  }
  static void classes(int num_class, float prior, float free_thresh, float occupied_thresh) {
    Semantics::num_class = num_class;
    Semantics::prior = prior;
    Semantics::free_thresh = free_thresh;
    Semantics::occupied_thresh = occupied_thresh;
  }
  static const std::vector<float>& ms(const Semantics& s) { return s.ms; }
  static const std::vector<float>& fs(const Semantics& s) { return s.fs; }

  typedef RTree<Hit*, float, 3, float> Tree;
  static bool collect(Hit* h, void* out) {
    static_cast<std::vector<Hit*>*>(out)->push_back(h);
    return true;
  }
  static void in_box(Tree& rtree, BlockHashKey key, std::vector<Hit*>& out) {
    const float block_size = Block::size;
    point3f half_size(block_size / 2.0f, block_size / 2.0f, block_size / 2.0);
    point3f lim_min = hash_key_to_block(key) - half_size;
    point3f lim_max = hash_key_to_block(key) + half_size;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = lim_min(a), hi[a] = lim_max(a);
    out.clear();
    rtree.Search(lo, hi, collect, &out);
  }
};

}  // namespace semantic_bki

using namespace semantic_bki;
typedef SemanticBKIOctoMap Map;

static std::vector<uint32_t> in, out;
static size_t at = 0;

static uint32_t word() {
  if (at >= in.size()) {
    fprintf(stderr, "bki_upstream: the case file ends inside an operation\n");
    exit(3);
  }
  return in[at++];
}
static float real() {
  uint32_t w = word();
  float f;
  memcpy(&f, &w, 4);
  return f;
}
static void put(uint32_t w) { out.push_back(w); }
static void put(float f) {
  uint32_t w;
  memcpy(&w, &f, 4);
  out.push_back(w);
}
static void put_key(BlockHashKey k) {
  put((uint32_t)((uint64_t)k & 0xFFFFFFFFu));
  put((uint32_t)((uint64_t)k >> 32));
}
static void put(const std::vector<float>& v) {
  for (float f : v) put(f);
}
static void put(const point3f& p) {
  put(p.x());
  put(p.y());
  put(p.z());
}

// the keys of the 5 x 5 x 5 blocks around `key` that the key's fields can hold
static std::vector<BlockHashKey> around(BlockHashKey key) {
  const int64_t k[3] = {key >> 40, (key >> 20) & 0xFFFFF, key & 0xFFFFF};
  std::vector<BlockHashKey> r;
  for (int64_t x = k[0] - 2; x <= k[0] + 2; ++x)
    for (int64_t y = k[1] - 2; y <= k[1] + 2; ++y)
      for (int64_t z = k[2] - 2; z <= k[2] + 2; ++z)
        if (x >= 0 && y >= 0 && z >= 0 && x <= 0xFFFFF && y <= 0xFFFFF && z <= 0xFFFFF) r.push_back((x << 40) | (y << 20) | z);
  return r;
}

static void read_points(std::vector<Hit>& hits, uint32_t n, bool rows) {
  hits.resize(n);
  for (Hit& h : hits) {
    for (float& c : h.p) c = real();
    h.cls = rows ? word() : 0;
    h.has_row = rows ? word() : 0;
    for (float& f : h.row) f = rows ? real() : 0.0f;
  }
}

static void fill(Map::Tree& rtree, std::vector<Hit>& hits) {
  for (Hit& h : hits) rtree.Insert(h.p, h.p, &h);
}

static void op_keys() {
  Map::grid(real());
  std::vector<Hit> hits;
  read_points(hits, word(), false);
  for (const Hit& h : hits) {
    BlockHashKey key = block_to_hash_key(h.p[0], h.p[1], h.p[2]);
    point3f centre = hash_key_to_block(key);
    Block block(centre);
    put_key(key);
    put(centre);
    put(block.get_loc(block.begin_leaf()));
  }
}

static void op_members() {
  Map::grid(real());
  std::vector<Hit> hits;
  read_points(hits, word(), false);
  Map::Tree rtree;
  fill(rtree, hits);
  std::vector<Hit*> found;
  for (Hit& h : hits) {
    std::vector<BlockHashKey> holding;
    for (BlockHashKey key : around(block_to_hash_key(h.p[0], h.p[1], h.p[2]))) {
      Map::in_box(rtree, key, found);
      for (Hit* f : found)
        if (f == &h) holding.push_back(key);
    }
    put((uint32_t)holding.size());
    for (BlockHashKey key : holding) put_key(key);
  }
}

static void put_read_outs(const Semantics& node, int num_class, bool with_probs) {
  std::vector<float> probs(num_class), occupied(num_class - 1), features(5);
  node.get_probs(probs);
  node.get_occupied_probs(occupied);
  node.get_features(features);
  if (with_probs) put(probs);
  if (with_probs) put(occupied);
  put(features);
  if (!with_probs) put(occupied);
}

static void op_node() {
  const int num_class = (int)word();
  const float prior = real(), free_thresh = real(), occupied_thresh = real();
  Map::classes(num_class, prior, free_thresh, occupied_thresh);
  Map::grid(0.5f);
  Block block(point3f(0.0f, 0.0f, 0.0f));
  Semantics& node = block.begin_leaf().get_node();
  for (uint32_t steps = word(); steps; --steps) {
    std::vector<float> ybars(num_class), fbars(5);
    for (float& y : ybars) y = real();
    for (float& f : fbars) f = real();
    node.update(ybars, fbars);
    put(Map::ms(node));
    put(Map::fs(node));
    put((uint32_t)node.get_state());
    put((uint32_t)node.get_semantics());
    put_read_outs(node, num_class, true);
  }
}

static void op_insert() {
  Map::grid(real());
  const int num_class = (int)word();
  const float prior = real(), free_thresh = real(), occupied_thresh = real();
  Map::classes(num_class, prior, free_thresh, occupied_thresh);
  std::map<BlockHashKey, Block*> blocks;
  for (uint32_t frames = word(); frames; --frames) {
    std::vector<Hit> hits;
    read_points(hits, word(), true);
    Map::Tree rtree;
    fill(rtree, hits);
    std::set<BlockHashKey> candidates, updated;
    for (const Hit& h : hits)
      for (BlockHashKey key : around(block_to_hash_key(h.p[0], h.p[1], h.p[2]))) candidates.insert(key);
    std::vector<Hit*> found;
    for (BlockHashKey key : candidates) {
      Map::in_box(rtree, key, found);
      if (found.size() < 1) continue;
      std::vector<float> ybars(num_class, 0.0f), fbars(5, 0.0f);
      for (const Hit* f : found) {
        ybars[f->cls] += 1.0f;
        if (f->has_row)
          for (int i = 0; i < 5; ++i) fbars[i] += f->row[i];
      }
      if (!blocks.count(key)) blocks[key] = new Block(hash_key_to_block(key));
      blocks[key]->begin_leaf().get_node().update(ybars, fbars);
      updated.insert(key);
    }
    put((uint32_t)blocks.size());
    for (const auto& kb : blocks) {
      const Block& block = *kb.second;
      auto leaf = block.begin_leaf();
      const Semantics& node = leaf.get_node();
      put_key(kb.first);
      put((uint32_t)updated.count(kb.first));
      put(Map::ms(node));
      put(Map::fs(node));
      put((uint32_t)node.get_state());
      put(block.get_loc(leaf));
      put_read_outs(node, num_class, false);
    }
  }
  for (auto& kb : blocks) delete kb.second;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: bki_upstream CASES RESULTS\n");
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t buf[4096];
  for (size_t n; (n = fread(buf, 4, 4096, f)) > 0;) in.insert(in.end(), buf, buf + n);
  fclose(f);
  while (at < in.size()) {
    switch (word()) {
      case 1: op_keys(); break;
      case 2: op_members(); break;
      case 3: op_node(); break;
      case 4: op_insert(); break;
      default: fprintf(stderr, "bki_upstream: unknown operation at word %zu\n", at - 1); return 3;
    }
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
