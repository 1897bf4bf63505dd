// cvo_lidar.hip -- LiDAR front end: cvo_lidar_select (CvoPointCloud(PointCloud<PointXYZI>::Ptr, n, beams, LOAM)'s point
// selection: LidarPointSelector::edge_detection, then LeGoLoamPointSelection::cloudHandler), cvo_lidar_select_host (the same
// on one CPU thread, no context), cvo_cloud_upload_lidar (the constructor's rows through the ordinary upload), the
// generator behind std::rand() and cvo_debug_lidar_stats.  tests/np_lidar.py states what is computed and where it departs
// from upstream's text.  On the device (cvo_k_lidar.h) only the n x 4 floats of the scan go up and only indices come back:
// the picks per ring and sixth and the thinned points ascending, which the host interleaves.  edge_detection is a serial
// walk (its ring state machine does not restart) over the host's copy of the scan: it runs on the calling thread on either
// route, on the device route while the kernels run.  A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// points; below, the CPU twin is faster than the launches: 8192 points 0.28 ms against 0.40, 16384 points 0.67 against 0.46
// (profiles/lidar/crossover.txt)
constexpr int LIDAR_HOST_BELOW = 12000;

bool lidar_on_host(const cvo_ctx* ctx, int n) { return route_on_host(ctx->opt.lidar_host, n, LIDAR_HOST_BELOW); }

// ---- glibc's TYPE_3 random(): r[i] += r[i - 3] over 31 words, the result without its lowest bit ----
unsigned lidar_rand_next(cvo_lidar_rand_t* s) {
  const unsigned v = (s->r[s->front] += s->r[s->rear]);
  if (++s->front >= 31) {
    s->front = 0;
    ++s->rear;
  } else if (++s->rear >= 31) {
    s->rear = 0;
  }
  return v >> 1;
}

void lidar_rand_seed(cvo_lidar_rand_t* s, unsigned seed) {
  if (seed == 0) seed = 1;
  int32_t word = (int32_t)seed;
  s->r[0] = seed;
  for (int i = 1; i < 31; i++) {  // the Lehmer generator 16807 x mod (2^31 - 1), by Schrage's division
    const int32_t hi = word / 127773, lo = word % 127773;
    word = 16807 * lo - 2836 * hi;
    if (word < 0) word += 2147483647;
    s->r[i] = (unsigned)word;
  }
  s->front = 3;
  s->rear = 0;
  for (int i = 0; i < 310; i++) (void)lidar_rand_next(s);
}

void lidar_derive(cvo_lidar_config_t* c) {
  const double deg = 3.14159265358979323846 / 180.0, m = (double)c->sensor_mount_angle;
  c->tan_theta = std::tan((double)c->segment_theta);
  c->sin_alpha_x = std::sin((double)c->segment_alpha_x);
  c->cos_alpha_x = std::cos((double)c->segment_alpha_x);
  c->sin_alpha_y = std::sin((double)c->segment_alpha_y);
  c->cos_alpha_y = std::cos((double)c->segment_alpha_y);
  c->tan_ground_lo = std::tan((m - 10.0) * deg);
  c->tan_ground_hi = std::tan((m + 10.0) * deg);
  c->tan_self_lo = std::tan((m - 3.0) * deg);
  c->tan_self_hi = std::tan((m + 3.0) * deg);
}

LidarConst lidar_const(const cvo_lidar_config_t& c) {
  LidarConst k;
  k.R = c.n_scan;
  k.H = c.horizon_scan;
  k.ground_rows = c.ground_scan_ind;
  k.valid_points = c.segment_valid_point_num;
  k.valid_lines = c.segment_valid_line_num;
  k.ang_res_x = c.ang_res_x;
  k.min_range = c.sensor_min_range;
  k.edge_thr = c.edge_threshold;
  k.tan_theta = c.tan_theta;
  k.sin_ax = c.sin_alpha_x;
  k.cos_ax = c.cos_alpha_x;
  k.sin_ay = c.sin_alpha_y;
  k.cos_ay = c.cos_alpha_y;
  k.tan_g_lo = c.tan_ground_lo;
  k.tan_g_hi = c.tan_ground_hi;
  k.tan_s_lo = c.tan_self_lo;
  k.tan_s_hi = c.tan_self_hi;
  return k;
}

int lidar_validate(const cvo_lidar_scan_t* s, const cvo_lidar_config_t* c, const cvo_lidar_rand_t* rand, std::string* msg) {
  auto bad = [&](const std::string& m) {
    *msg = m;
    return CVO_E_INVALID;
  };
  if (!s) return bad("scan is NULL");
  if (!c) return bad("config is NULL");
  if (!rand) return bad("rand is NULL");
  if (!s->xyzi) return bad("xyzi is NULL");
  if (s->n < 1) return bad("n must be at least 1, got " + std::to_string(s->n));
  if (s->num_classes < 0 || (s->num_classes > 0) != (s->semantic != nullptr))
    return bad("semantic and num_classes go together, got num_classes " + std::to_string(s->num_classes));
  if ((unsigned)rand->front >= 31u || (unsigned)rand->rear >= 31u) return bad("rand is not seeded (cvo_lidar_rand_seed)");
  if (c->n_scan < 1 || c->n_scan > LIDAR_MAX_SCAN) return bad("n_scan must be in 1 .. 128, got " + std::to_string(c->n_scan));
  if (c->horizon_scan < 1 || c->horizon_scan > LIDAR_MAX_HORIZON) return bad("horizon_scan must be in 1 .. 4096, got " + std::to_string(c->horizon_scan));
  if (c->ground_scan_ind < 0 || c->ground_scan_ind >= c->n_scan)
    return bad("ground_scan_ind must be in 0 .. n_scan - 1, got " + std::to_string(c->ground_scan_ind));
  auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  if (!pos(c->ang_res_x)) return bad("ang_res_x must be finite and > 0");
  if (!pos(c->sensor_min_range)) return bad("sensor_min_range must be finite and > 0");
  if (!(std::fabs(c->sensor_mount_angle) <= 45.f)) return bad("sensor_mount_angle must be within 45 degrees of 0");
  const float half_pi = 1.5707963f;
  if (!pos(c->segment_theta) || !(c->segment_theta < half_pi)) return bad("segment_theta must be in (0, pi / 2)");
  if (!pos(c->segment_alpha_x) || !(c->segment_alpha_x < half_pi) || !pos(c->segment_alpha_y) || !(c->segment_alpha_y < half_pi))
    return bad("segment_alpha_x and segment_alpha_y must be in (0, pi / 2)");
  if (c->segment_valid_point_num < 1 || c->segment_valid_line_num < 1) return bad("segment_valid_point_num and segment_valid_line_num must be positive");
  if (!pos(c->edge_threshold) || !pos(c->surf_threshold)) return bad("edge_threshold and surf_threshold must be finite and > 0");
  if (!pos(c->intensity_bound) || !pos(c->depth_bound) || !pos(c->distance_bound)) return bad("intensity_bound, depth_bound and distance_bound must be finite and > 0");
  if (c->beam_num < 1) return bad("beam_num must be positive, got " + std::to_string(c->beam_num));
  cvo_lidar_config_t d = *c;
  lidar_derive(&d);
  if (d.tan_theta != c->tan_theta || d.sin_alpha_x != c->sin_alpha_x || d.cos_alpha_x != c->cos_alpha_x || d.sin_alpha_y != c->sin_alpha_y ||
      d.cos_alpha_y != c->cos_alpha_y || d.tan_ground_lo != c->tan_ground_lo || d.tan_ground_hi != c->tan_ground_hi || d.tan_self_lo != c->tan_self_lo ||
      d.tan_self_hi != c->tan_self_hi)
    return bad("the derived fields do not match the angles (cvo_lidar_config_derive)");
  if (s->n > LIDAR_MAX_POINTS) {
    *msg = "more than 2^24 points";
    return CVO_E_UNSUPPORTED;
  }
  for (size_t i = 0; i < 4 * (size_t)s->n; i++) {
    const float v = s->xyzi[i];
    if ((i & 3) == 3 ? !std::isfinite(v) : !(std::fabs(v) < 1e15f)) return bad("point " + std::to_string(i / 4) + " has a non-finite (or, in magnitude, 1e15 or larger) value");
  }
  if (s->semantic)
    for (int i = 0; i < s->n; i++)
      if (s->semantic[i] < -1 || s->semantic[i] >= s->num_classes) return bad("semantic[" + std::to_string(i) + "] is outside -1 .. num_classes - 1");
  return CVO_OK;
}

// ---- LidarPointSelector::edge_detection: a serial walk on either route ----
void lidar_edge_detection(const cvo_lidar_scan_t& s, const cvo_lidar_config_t& c, std::vector<int>& out) {
#pragma clang fp contract(off)
  const float* p = s.xyzi;
  const int n = s.n;
  int prev = lidar_quadrant(p[0], p[2]), ring = 0;
  for (int i = 1; i < n - 1; i++) {
    if (s.semantic && s.semantic[i] == -1) continue;
    const float* a = p + 4 * (size_t)(i - 1);
    const float* b = a + 4;
    const float* d = b + 4;
    const int quadrant = lidar_quadrant(b[0], b[2]);
    if (quadrant == 1 && prev == 4 && ring < c.beam_num - 1) {
      ring++;
      continue;  // (prev stays 4: upstream's `continue` skips its update)
    }
    const float lx = a[0] - b[0], ly = a[1] - b[1], lz = a[2] - b[2], rx = b[0] - d[0], ry = b[1] - d[1], rz = b[2] - d[2];
    const float nl = lidar_sqrtf(lx * lx + ly * ly + lz * lz), nr = lidar_sqrtf(rx * rx + ry * ry + rz * rz);
    const double depth_grad = (double)(nl > nr ? nl : nr);
    const float il = std::fabs(a[3] - b[3]), ir = std::fabs(b[3] - d[3]);
    const double intensity_grad = (double)(il > ir ? il : ir);
    if ((intensity_grad > c.intensity_bound || depth_grad > c.depth_bound) && b[3] > 0.f && b[0] != 0.f && b[1] != 0.f && b[2] != 0.f &&
        (double)lidar_range(b[0], b[1], b[2]) < c.distance_bound)
      out.push_back(i);
    prev = quadrant;
  }
}

// what either route leaves of cloudHandler: point indices in upstream's order, 1 for its edges
struct LidarLego {
  std::vector<int> index;
  std::vector<unsigned char> is_edge;
};

// ---- CPU twin of cloudHandler ----
void lidar_lego_cpu(const cvo_lidar_scan_t& s, const LidarConst& k, cvo_lidar_rand_t* rand, LidarLego& out, LidarStatsAcc& st) {
  const float* p = s.xyzi;
  const int n = s.n, R = k.R, H = k.H, cells = R * H;
  // copyPointCloud + projectPointCloud: the last point in index order wins its cell
  std::vector<int> win((size_t)cells, -1);
  std::vector<float> range((size_t)cells, FLT_MAX);
  int ring = 0, prev = lidar_quadrant(p[0], p[2]);
  for (int i = 0; i < n; i++) {
    const float* q = p + 4 * (size_t)i;
    const int quadrant = lidar_quadrant(q[0], q[2]);
    if (quadrant == 1 && prev == 4) ring++;
    prev = quadrant;
    if (ring >= R) continue;
    const int col = lidar_column(q[0], q[2], k.ang_res_x, H);
    if (col < 0) continue;
    const float r = lidar_range(q[0], q[1], q[2]);
    if (r < k.min_range) continue;
    win[(size_t)ring * H + col] = i;
    range[(size_t)ring * H + col] = r;
  }
  // groundRemoval
  std::vector<signed char> ground((size_t)cells, 0);
  for (int j = 0; j < H; j++)
    for (int i = 0; i < k.ground_rows; i++) {
      const int lo = j + i * H, up = lo + H;
      if (win[lo] < 0 || win[up] < 0) continue;
      if (lidar_ground_pair(p + 4 * (size_t)win[lo], p + 4 * (size_t)win[up], k)) ground[lo] = ground[up] = 1;
    }
  std::vector<int> label((size_t)cells, 0);
  for (int c = 0; c < cells; c++) {
    if (win[c] >= 0) st.projected++;
    if (ground[c]) st.ground++;
    if (ground[c] || win[c] < 0) label[c] = -1;
  }
  // cloudSegmentation: labelComponents from every unlabelled cell in row-major order
  const int INVALID = 999999;
  int label_count = 1;
  std::vector<int> queue((size_t)cells);
  static const int step[4][2] = {{-1, 0}, {0, 1}, {0, -1}, {1, 0}};
  for (int seed = 0; seed < cells; seed++) {
    if (label[seed] != 0) continue;
    unsigned mask[4] = {0, 0, 0, 0};
    int head = 0, tail = 0;
    queue[tail++] = seed;
    label[seed] = label_count;
    while (head < tail) {
      const int from = queue[head++], fr = from / H, fc = from - fr * H;
      for (const auto& d : step) {
        const int r = fr + d[0];
        int c = fc + d[1];
        if (r < 0 || r >= R) continue;
        if (c < 0) c = H - 1;
        if (c >= H) c = 0;
        const int to = r * H + c;
        if (label[to] != 0) continue;
        if (!lidar_connected(range[from], range[to], d[0] == 0, k)) continue;
        queue[tail++] = to;
        label[to] = label_count;
        mask[r >> 5] |= 1u << (r & 31);
      }
    }
    if (lidar_segment_valid((unsigned)tail, mask, k)) {
      label_count++;
      st.valid++;
    } else {
      for (int t = 0; t < tail; t++) label[queue[t]] = INVALID;
      st.invalid++;
    }
  }
  // the segmented cloud (ground cells carry label -1: none of them enters, so no flat-surface pick can happen)
  std::vector<int> seg_col, seg_pt, before((size_t)R + 1, 0);
  std::vector<float> seg_range;
  for (int i = 0; i < R; i++) {
    before[i] = (int)seg_pt.size();
    for (int j = 0; j < H; j++) {
      const int c = i * H + j;
      if (label[c] > 0 && label[c] != INVALID) {
        seg_col.push_back(j);
        seg_pt.push_back(win[c]);
        seg_range.push_back(range[c]);
      }
    }
  }
  const int S = (int)seg_pt.size();
  before[R] = S;
  st.segmented = (unsigned long long)S;
  // calculateSmoothness, markOccludedPoints
  std::vector<float> curv((size_t)S);
  std::vector<unsigned char> picked((size_t)S), edge((size_t)S, 0);
  for (int i = 0; i < S; i++) {
    curv[i] = lidar_curvature(seg_range.data(), i, S);
    picked[i] = lidar_occluded(seg_range.data(), seg_col.data(), i, S) ? 1 : 0;
  }
  // extractFeatures
  std::vector<std::pair<float, int>> sm;
  for (int i = 0; i < R; i++)
    for (int j = 0; j < LIDAR_SIXTHS; j++) {
      int sp, ep;
      lidar_sixth(before[i], before[i + 1], j, &sp, &ep);
      if (sp >= ep) continue;
      sm.clear();
      for (int t = sp; t <= ep; t++) sm.push_back(t >= 5 && t < S - 5 ? std::make_pair(curv[t], t) : std::make_pair(0.f, 0));
      std::sort(sm.begin(), sm.end() - 1);  // [sp, ep): by (value, index)
      int cnt = 0;
      for (int t = ep - sp; t >= 0; t--) {
        const int ind = sm[(size_t)t].second;
        if (picked[ind] || !(curv[ind] > k.edge_thr)) continue;
        if (++cnt > LIDAR_EDGE_CAP) break;
        edge[ind] = 1;
        out.index.push_back(seg_pt[ind]);
        out.is_edge.push_back(1);
        st.edges++;
        picked[ind] = 1;
        for (int l = 1; l <= 5; l++) {
          if (lidar_col_gap(seg_col.data(), ind + l, ind + l - 1) > 10) break;
          picked[ind + l] = 1;
        }
        for (int l = -1; l >= -5; l--) {
          if (lidar_col_gap(seg_col.data(), ind + l, ind + l + 1) > 10) break;
          picked[ind + l] = 1;
        }
      }
      for (int t = sp; t <= ep; t++)
        if (!edge[t]) {
          st.draws++;
          if (lidar_rand_next(rand) % 4 == 0) {
            out.index.push_back(seg_pt[t]);
            out.is_edge.push_back(0);
            st.thinned++;
          }
        }
    }
}

// ---- device route of cloudHandler ----
struct LidarDevice {
  float4* pts;
  unsigned* blocks;
  unsigned* ctl;  // [4] totals: transitions, segmented points, draws, thinned points
  char *zero, *zero_end;  // stats, size, mask, cand, kept: cleared together
  LidarStats* stats;
  unsigned *size, *mask;
  unsigned char *cand, *kept, *state, *valid, *occluded, *quarter;
  int *cellwin, *parent, *root, *seg_cell, *seg_col, *seg_pt, *before, *edge_pt, *n_edge, *out_k, *out_pt;
  float *range, *seg_range, *curv;
};

int lidar_device_layout(cvo_ctx* ctx, int n, const LidarConst& k, LidarDevice& d) {
  const size_t cells = (size_t)k.R * k.H, nb = (std::max((size_t)n, cells) + COMPACT_THREADS - 1) / COMPACT_THREADS;
  return ctx->lidar_scratch.lay_out(ctx, "LiDAR scratch", [&](ScratchLayout& l) {
    l.take(d.pts, (size_t)n);
    l.take(d.blocks, nb);
    l.take(d.ctl, 4);
    l.at(d.zero, l.off);
    l.take(d.stats, 1);
    l.take(d.size, cells);
    l.take(d.mask, 4 * cells);  // (four words of row bits per cell)
    l.take(d.cand, cells);
    l.take(d.kept, cells);
    l.at(d.zero_end, l.off);
    l.take(d.state, cells);
    l.take(d.valid, cells);
    l.take(d.occluded, cells);
    l.take(d.quarter, cells);
    l.take(d.cellwin, cells);
    l.take(d.parent, cells);
    l.take(d.root, cells);
    l.take(d.seg_cell, cells);
    l.take(d.seg_col, cells);
    l.take(d.seg_pt, cells);
    l.take(d.before, (size_t)k.R + 1);
    l.take(d.edge_pt, (size_t)k.R * LIDAR_SIXTHS * LIDAR_EDGE_CAP);
    l.take(d.n_edge, (size_t)k.R * LIDAR_SIXTHS);
    l.take(d.out_k, cells);
    l.take(d.out_pt, cells);
    l.take(d.range, cells);
    l.take(d.seg_range, cells);
    l.take(d.curv, cells);
  });
}

// `between`: host work that needs no device result (edge_detection), run while the range-image kernels do
template <class Between>
int lidar_lego_device(cvo_ctx* ctx, const cvo_lidar_scan_t& s, const LidarConst& k, cvo_lidar_rand_t* rand, LidarLego& out, LidarStatsAcc& st,
                      Between between) {
  const char* who = "cvo_lidar_select";
  const int n = s.n, cells = k.R * k.H, cell_blocks = (cells + LIDAR_THREADS - 1) / LIDAR_THREADS;
  hipStream_t q = ctx->upload_stream;
  LidarDevice d;
  int rc = lidar_device_layout(ctx, n, k, d);
  if (rc != CVO_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d.pts, s.xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, q));
  HIP_TRY(ctx, hipMemsetAsync(d.zero, 0, (size_t)(d.zero_end - d.zero), q));
  HIP_TRY(ctx, hipMemsetAsync(d.cellwin, 0xff, sizeof(int) * (size_t)cells, q));
  const LidarTransition tr{d.pts};
  const int nbp = (n + COMPACT_THREADS - 1) / COMPACT_THREADS;
  hipLaunchKernelGGL(k_compact_count<LidarTransition>, dim3(nbp), dim3(COMPACT_THREADS), 0, q, n, tr, d.blocks);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(COMPACT_THREADS), 0, q, nbp, d.blocks, d.ctl + 0);
  hipLaunchKernelGGL(k_lidar_project, dim3(nbp), dim3(COMPACT_THREADS), 0, q, n, tr, k, (const unsigned*)d.blocks, d.cellwin);
  hipLaunchKernelGGL(k_lidar_cells, dim3(cell_blocks), dim3(LIDAR_THREADS), 0, q, k, (const float4*)d.pts, (const int*)d.cellwin, d.range, d.state, d.parent,
                     d.stats);
  hipLaunchKernelGGL(k_lidar_union, dim3(cell_blocks), dim3(LIDAR_THREADS), 0, q, k, (const float*)d.range, (const unsigned char*)d.state, d.parent);
  hipLaunchKernelGGL(k_lidar_flatten, dim3(cell_blocks), dim3(LIDAR_THREADS), 0, q, k, (const unsigned char*)d.state, d.parent, d.root, d.size, d.mask);
  hipLaunchKernelGGL(k_lidar_valid, dim3(cell_blocks), dim3(LIDAR_THREADS), 0, q, k, (const int*)d.root, (const unsigned*)d.size, (const unsigned*)d.mask,
                     d.valid, d.stats);
  HIP_TRY(ctx, hipGetLastError());
  const LidarSegKeep seg_keep{k.H, d.valid, d.range, d.cellwin, d.seg_cell, d.seg_col, d.seg_pt, d.seg_range};
  if ((rc = compact(ctx, cells, seg_keep, d.blocks, scan_into(ctx, d.ctl + 1))) != CVO_OK) return rc;
  between();
  unsigned seg = 0;
  if ((rc = compact_total(ctx, d.ctl + 1, cells, who, "range-image cells", &seg)) != CVO_OK) return rc;
  const int S = (int)seg;
  std::vector<int> before((size_t)k.R + 1, 0), n_edge((size_t)k.R * LIDAR_SIXTHS, 0), edge_pt((size_t)k.R * LIDAR_SIXTHS * LIDAR_EDGE_CAP), out_k, out_pt;
  std::vector<unsigned char> quarter((size_t)S);
  unsigned ctl[4] = {};
  LidarStats hs{};
  cvo_lidar_rand_t ahead = *rand;
  if (S > 0) {
    for (int t = 0; t < S; t++) quarter[(size_t)t] = (unsigned char)(lidar_rand_next(&ahead) % 4);  // the next S draws: no call consumes more
    HIP_TRY(ctx, hipMemcpyAsync(d.quarter, quarter.data(), (size_t)S, hipMemcpyHostToDevice, q));
    const int seg_blocks = (S + LIDAR_THREADS - 1) / LIDAR_THREADS;
    hipLaunchKernelGGL(k_lidar_bounds, dim3((k.R + 1 + LIDAR_THREADS - 1) / LIDAR_THREADS), dim3(LIDAR_THREADS), 0, q, k.R, k.H, S, (const int*)d.seg_cell,
                       d.before);
    hipLaunchKernelGGL(k_lidar_smooth, dim3(seg_blocks), dim3(LIDAR_THREADS), 0, q, S, (const float*)d.seg_range, (const int*)d.seg_col, d.curv, d.occluded);
    hipLaunchKernelGGL(k_lidar_pick, dim3(k.R), dim3(LIDAR_PICK_THREADS), 0, q, S, k.edge_thr, (const int*)d.before, (const float*)d.curv,
                       (const unsigned char*)d.occluded, (const int*)d.seg_col, (const int*)d.seg_pt, d.edge_pt, d.n_edge, d.cand);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = compact(ctx, S, LidarCand{d.cand, d.quarter, d.kept}, d.blocks, scan_into(ctx, d.ctl + 2))) != CVO_OK) return rc;
    if ((rc = compact(ctx, S, LidarKept{d.kept, d.seg_pt, d.out_k, d.out_pt}, d.blocks, scan_into(ctx, d.ctl + 3))) != CVO_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(before.data(), d.before, sizeof(int) * before.size(), hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipMemcpyAsync(n_edge.data(), d.n_edge, sizeof(int) * n_edge.size(), hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipMemcpyAsync(edge_pt.data(), d.edge_pt, sizeof(int) * edge_pt.size(), hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipMemcpyAsync(ctl, d.ctl, sizeof ctl, hipMemcpyDeviceToHost, q));
  }
  HIP_TRY(ctx, hipMemcpyAsync(&hs, d.stats, sizeof hs, hipMemcpyDeviceToHost, q));
  HIP_TRY(ctx, hipStreamSynchronize(q));
  const unsigned draws = ctl[2], thinned = ctl[3];
  if (draws > (unsigned)S || thinned > draws) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device kept more candidates than it was given");
  out_k.resize(thinned);
  out_pt.resize(thinned);
  if (thinned) {
    HIP_TRY(ctx, hipMemcpyAsync(out_k.data(), d.out_k, sizeof(int) * thinned, hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipMemcpyAsync(out_pt.data(), d.out_pt, sizeof(int) * thinned, hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipStreamSynchronize(q));
  }
  // per ring and sixth: the edges in pick order, then the thinned points of its range (both lists ascend with the ranges)
  size_t at = 0;
  for (int i = 0; i < k.R; i++) {
    if (before[(size_t)i] > before[(size_t)i + 1] || before[(size_t)i + 1] > S) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device's ring bounds do not ascend");
    for (int j = 0; j < LIDAR_SIXTHS; j++) {
      int sp, ep;
      lidar_sixth(before[(size_t)i], before[(size_t)i + 1], j, &sp, &ep);
      if (sp >= ep) continue;
      const int ne = n_edge[(size_t)i * LIDAR_SIXTHS + j];
      if (ne < 0 || ne > LIDAR_EDGE_CAP) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device picked more edges than a sixth holds");
      for (int t = 0; t < ne; t++) {
        const int pt = edge_pt[((size_t)i * LIDAR_SIXTHS + j) * LIDAR_EDGE_CAP + t];
        if ((unsigned)pt >= (unsigned)n) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device picked a point outside the scan");
        out.index.push_back(pt);
        out.is_edge.push_back(1);
      }
      st.edges += (unsigned long long)ne;
      for (; at < out_k.size() && out_k[at] <= ep; at++) {
        if (out_k[at] < sp || (unsigned)out_pt[at] >= (unsigned)n) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device kept a point outside its sixth");
        out.index.push_back(out_pt[at]);
        out.is_edge.push_back(0);
      }
    }
  }
  if (at != out_k.size()) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device kept a point outside every sixth");
  for (unsigned t = 0; t < draws; t++) (void)lidar_rand_next(rand);
  st.projected = hs.projected;
  st.ground = hs.ground;
  st.valid = hs.valid;
  st.invalid = hs.invalid;
  st.segmented = (unsigned long long)S;
  st.draws = draws;
  st.thinned = thinned;
  return CVO_OK;
}

// both lists, by the route `ctx` takes (nullptr: the twin); with semantics LeGO-LOAM's unlabelled points drop out here
int lidar_select_any(cvo_ctx* ctx, const cvo_lidar_scan_t& s, const cvo_lidar_config_t& c, cvo_lidar_rand_t* rand, std::vector<int>& index,
                     std::vector<unsigned char>& is_edge, LidarStatsAcc& st) {
  const LidarConst k = lidar_const(c);
  LidarLego lego;
  index.clear();
  if (!ctx || lidar_on_host(ctx, s.n)) {
    lidar_edge_detection(s, c, index);
    lidar_lego_cpu(s, k, rand, lego, st);
  } else {
    st.on_device = 1;
    const int rc = lidar_lego_device(ctx, s, k, rand, lego, st, [&] { lidar_edge_detection(s, c, index); });
    if (rc != CVO_OK) return rc;
  }
  st.edge_detected = index.size();
  is_edge.assign(index.size(), 1);
  for (size_t i = 0; i < lego.index.size(); i++) {
    if (s.semantic && s.semantic[lego.index[i]] == -1) continue;
    index.push_back(lego.index[i]);
    is_edge.push_back(lego.is_edge[i]);
  }
  return CVO_OK;
}

void lidar_copy_out(const std::vector<int>& index, const std::vector<unsigned char>& edge, int* out, unsigned char* is_edge, int* n) {
  if (out && !index.empty()) std::memcpy(out, index.data(), sizeof(int) * index.size());
  if (is_edge && !edge.empty()) std::memcpy(is_edge, edge.data(), edge.size());
  if (n) *n = (int)index.size();
}

// the refusals every entry point shares (a twin, ctx == nullptr, stores no text)
int lidar_check(cvo_ctx* ctx, const char* who, const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, const cvo_lidar_rand_t* rand) {
  std::string msg;
  const int rc = lidar_validate(scan, cfg, rand, &msg);
  return rc != CVO_OK ? fail(ctx, rc, std::string(who) + ": " + msg) : rc;
}

// the body of cvo_lidar_select_host and cvo_lidar_select; *rand moves on only when the call succeeds
int lidar_select_entry(cvo_ctx* ctx, const char* who, const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand, int* index,
                       unsigned char* is_edge, int* n) {
  const int rc = lidar_check(ctx, who, scan, cfg, rand);
  if (rc != CVO_OK) return rc;
  if (!index || !n) return fail(ctx, CVO_E_INVALID, std::string(who) + ": index and n are required");
  return frontend_call(ctx, who, [&] {
    std::vector<int> idx;
    std::vector<unsigned char> edge;
    LidarStatsAcc st;
    cvo_lidar_rand_t r = *rand;
    const int rc = lidar_select_any(ctx, *scan, *cfg, &r, idx, edge, st);
    if (rc != CVO_OK) return rc;
    *rand = r;
    lidar_copy_out(idx, edge, index, is_edge, n);
    if (ctx) ctx->lidar_last = st;
    return CVO_OK;
  });
}

}  // namespace

extern "C" {

void cvo_lidar_config_derive(cvo_lidar_config_t* cfg) {
  if (cfg) lidar_derive(cfg);
}

void cvo_lidar_config_default(cvo_lidar_config_t* cfg, int semantic) {
  if (!cfg) return;
  const float ang_res_x = 0.2f, ang_res_y = 0.427f;
  cfg->n_scan = 64;
  cfg->horizon_scan = 1800;
  cfg->ang_res_x = ang_res_x;
  cfg->ground_scan_ind = 50;
  cfg->sensor_min_range = 1.0f;
  cfg->sensor_mount_angle = 0.0f;
  cfg->segment_theta = (float)(60.0 / 180.0 * 3.14159265358979323846);
  cfg->segment_alpha_x = (float)(ang_res_x / 180.0 * 3.14159265358979323846);
  cfg->segment_alpha_y = (float)(ang_res_y / 180.0 * 3.14159265358979323846);
  cfg->segment_valid_point_num = 5;
  cfg->segment_valid_line_num = 3;
  cfg->edge_threshold = 0.1f;
  cfg->surf_threshold = 0.1f;
  cfg->intensity_bound = 0.4;
  cfg->depth_bound = 4.0;
  cfg->distance_bound = semantic ? 75.0 : 40.0;
  cfg->beam_num = 64;
  lidar_derive(cfg);
}

void cvo_lidar_rand_seed(cvo_lidar_rand_t* state, unsigned int seed) {
  if (state) lidar_rand_seed(state, seed);
}

unsigned int cvo_lidar_rand_next(cvo_lidar_rand_t* state) {
  if (!state || (unsigned)state->front >= 31u || (unsigned)state->rear >= 31u) return 0;
  return lidar_rand_next(state);
}

int cvo_lidar_select_host(const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand, int* index, unsigned char* is_edge, int* n) {
  return lidar_select_entry(nullptr, "cvo_lidar_select_host", scan, cfg, rand, index, is_edge, n);
}

int cvo_lidar_select(cvo_ctx* ctx, const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand, int* index, unsigned char* is_edge,
                     int* n) {
  if (!ctx) return CVO_E_INVALID;
  return lidar_select_entry(ctx, "cvo_lidar_select", scan, cfg, rand, index, is_edge, n);
}

int cvo_cloud_upload_lidar(cvo_ctx* ctx, const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand, cvo_cloud** out, int* index,
                           int* n) {
  if (!ctx) return CVO_E_INVALID;
  const int rc = lidar_check(ctx, "cvo_cloud_upload_lidar", scan, cfg, rand);
  if (rc != CVO_OK) return rc;
  if (!out) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_lidar: out is NULL");
  return frontend_call(ctx, "cvo_cloud_upload_lidar", [&] {
    std::vector<int> idx;
    std::vector<unsigned char> edge;
    LidarStatsAcc st;
    cvo_lidar_rand_t r = *rand;
    int rc = lidar_select_any(ctx, *scan, *cfg, &r, idx, edge, st);
    if (rc != CVO_OK) return rc;
    // the constructor's rows: F = 1 (intensity) zero-padded to FD, type (1, 0), one-hot labels padded / cut to NC
    const size_t np = idx.size();
    const bool sem = scan->semantic != nullptr;
    std::vector<float> xyz(3 * np), feat((size_t)FD * np, 0.f), geo(2 * np), label(sem ? (size_t)NC * np : 0, 0.f);
    for (size_t i = 0; i < np; i++) {
      const float* p = scan->xyzi + 4 * (size_t)idx[i];
      std::memcpy(&xyz[3 * i], p, sizeof(float) * 3);
      feat[(size_t)FD * i] = p[3];
      geo[2 * i] = 1.f;
      geo[2 * i + 1] = 0.f;
      if (sem && scan->semantic[idx[i]] >= 0 && scan->semantic[idx[i]] < NC) label[(size_t)NC * i + scan->semantic[idx[i]]] = 1.f;
    }
    const HostCloud h{(int)np, (const char*)xyz.data(), 12, (const char*)feat.data(), sizeof(float) * FD, sem ? (const char*)label.data() : nullptr,
                      sizeof(float) * NC, (const char*)geo.data(), 8};
    if ((rc = upload_one_locked(ctx, h, out)) != CVO_OK) return rc;
    *rand = r;
    lidar_copy_out(idx, edge, index, nullptr, n);
    ctx->lidar_last = st;
    return CVO_OK;
  });
}

int cvo_debug_lidar_atan2(int n, const double* y, const double* x, double* out) {
  if (n < 0 || (n > 0 && (!y || !x || !out))) return CVO_E_INVALID;
  for (int i = 0; i < n; i++) out[i] = lidar_atan2_deg(y[i], x[i]);
  return CVO_OK;
}

int cvo_debug_lidar_stats(cvo_ctx* ctx, unsigned long long* counts, int* on_device) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const LidarStatsAcc& s = ctx->lidar_last;
  if (counts) {
    const unsigned long long v[9] = {s.projected, s.ground, s.valid, s.invalid, s.segmented, s.edges, s.draws, s.thinned, s.edge_detected};
    std::memcpy(counts, v, sizeof v);
  }
  if (on_device) *on_device = s.on_device;
  return CVO_OK;
}

}  // extern "C"
