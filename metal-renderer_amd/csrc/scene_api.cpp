// scene_api.cpp — the scene object of include/mrt.h (import, BVH build, the
// scene-detected shortcuts: occluder tree, convex solids, leaf-box sweep;
// upload), its checks and debug accessors, and the MPS-shaped mrt_accel over
// caller-owned buffers.  mrt_scene_create runs the stages below in order over
// one SceneBuild.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "host_internal.h"
#include "bvh_gpu.h"
#include "diag_env.h"
#include "occluders.h"
#include "sweep_pairs.h"

using namespace mrt::host;

namespace {

// What the stages of mrt_scene_create hand to one another; what outlives the
// build goes straight into the scene `s`.
struct SceneBuild {
  const mrt_scene_desc* desc = nullptr;
  mrt_scene* s = nullptr;
  uint32_t T = 0;                          // triangles (= primitives)
  uint32_t builder = 0;                    // MRT_BVH_*
  mrt::BvhBuildOptions opt;                // the main tree's, overrides applied
  double build_ms = 0.0;
  std::vector<float> prims, mats, lights;  // shading, material and light records
  std::vector<float> up_nodes, up_tris;    // nodes / leaf triangles as uploaded: the main tree's, then the occluder tree's
  mrt::OccluderSet occ;
  mrt::BvhResult ob;                       // the occluder tree
  bool occ_on = false;                     // shadow rays get an occluder tree (false again once it is dropped)
  bool occ_lights = false;                 // ... which leaves the light triangles out
  int32_t occ_root = mrt::kEmptyChild;
  mrt::ConvexSet conv;
  bool conv_on = false;
  uint32_t sweep_leaves = 0;               // records of the kernels' sweep list (sweep_pairs)
};

// stage 1: the main tree's build options from the descriptor, with their
// diagnostic overrides
int build_options(SceneBuild& b) {
  const mrt_scene_desc* desc = b.desc;
  mrt::BvhBuildOptions& opt = b.opt;
  if (desc->max_leaf_size) opt.max_leaf_size = desc->max_leaf_size;
  if (desc->lds_nodes == UINT32_MAX) opt.lds_node_budget = 0;
  else if (desc->lds_nodes) opt.lds_node_budget = desc->lds_nodes;
  else opt.lds_node_budget = 256;   // BFS prefix; the launcher stages what fits (fit_lds_nodes)
  if (const char* v = mrt::diag_env("MRT_LDS_NODES"); v && !desc->lds_nodes) opt.lds_node_budget = (uint32_t)std::strtoul(v, nullptr, 0);
  // large scenes (traversed from global memory): a finer SAH — 64 bins, and
  // the exact sweep for ranges below 64 K triangles: C4 1822 -> 1925-1935
  // Mpaths/s (+5.7 %, SAH cost 22.3 -> 20.5), C3 / C3g (7 K triangles) unchanged
  // (tools/env_sweep.sh, r2).  The presorted full sweep at every node
  // (MRT_FULL_SWEEP=1: SAH cost 19.0, the fastest build) measured C4 -1.1 %,
  // C5 share -1.0 %, C2 -2.5 % against it, so it is opt-in.
  if (b.T >= 65536) {
    opt.bins = 64;
    opt.exact_sah_below = 65536;
  }
  if (const char* v = mrt::diag_env("MRT_FULL_SWEEP")) opt.full_sweep = std::atoi(v) != 0;
  // tuning overrides (profiling): MRT_LEAF = max leaf size, MRT_CTRAV = SAH node cost
  if (const char* v = mrt::diag_env("MRT_LEAF")) opt.max_leaf_size = (uint32_t)std::strtoul(v, nullptr, 0);
  if (const char* v = mrt::diag_env("MRT_CTRAV")) opt.traversal_cost = std::strtof(v, nullptr);
  if (const char* v = mrt::diag_env("MRT_BINS")) opt.bins = (uint32_t)std::strtoul(v, nullptr, 0);
  if (const char* v = mrt::diag_env("MRT_EXACT_SAH")) opt.exact_sah_below = (uint32_t)std::strtoul(v, nullptr, 0);
  // BVH4 collapse: opt.collapse_dp's size policy (bvh.h), the same for every
  // build path — the area-optimal collapse below 64 K triangles: C2 +0.8 %,
  // C3 +1.9 %, C3g +0.5 %; the 1M-triangle C4 tree (21 % fewer, fuller
  // nodes: more children pushed per step) -1.2 %, so greedy there (r4)
  b.builder = desc->bvh_builder ? desc->bvh_builder : MRT_BVH_HOST_SAH;
  // BVH4 is the one layout the kernels traverse (BVH2 measured -24 %, a
  // compressed BVH8 -33 % and a quantised BVH4 -10 % on C4 in r2)
  opt.width = desc->bvh_width ? desc->bvh_width : 4;
  if (opt.width != 4) return fail(MRT_ERR_INVALID, "bvh_width must be 4 (or 0 = default)");
  if (b.builder != MRT_BVH_HOST_SAH && b.builder != MRT_BVH_DEVICE_LBVH && b.builder != MRT_BVH_DEVICE_PLOC)
    return fail(MRT_ERR_INVALID, "unknown bvh_builder");
  if (b.builder != MRT_BVH_HOST_SAH && desc->device < 0) return fail(MRT_ERR_INVALID, "device BVH build needs a device");
  return MRT_OK;
}

// stage 2: the main tree, built on the host or on the device (the only stage
// before the upload that touches HIP, and only for a device builder)
int build_main_tree(SceneBuild& b) {
  mrt_scene* s = b.s;
  const mrt::HostScene& h = s->host;
  std::string err;
  if (b.builder == MRT_BVH_HOST_SAH) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!mrt::build_bvh(h.vertices.data()->v, sizeof(mrt::RefVertex), h.indices.data(), b.T, b.opt, s->bvh, err))
      return fail(MRT_ERR_INVALID, "BVH build failed: " + err);
    b.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  } else {
    // MPS-style: the vertex and index buffers go to the device first and the
    // structure is built there (MPSTriangleAccelerationStructure.rebuild)
    HIP_TRY(hipSetDevice(b.desc->device));
    DevBuf dv, di;
    HIP_TRY(upload(dv, h.vertices.data(), h.vertices.size() * sizeof(mrt::RefVertex)));
    HIP_TRY(upload(di, h.indices.data(), h.indices.size() * 4));
    mrt::GpuBvhResult g;
    if (mrt::build_bvh_gpu(dv.as<float>(), sizeof(mrt::RefVertex), di.as<uint32_t>(), b.T, b.opt.max_leaf_size,
                           b.builder == MRT_BVH_DEVICE_PLOC ? mrt::GpuBvhAlgo::kPloc : mrt::GpuBvhAlgo::kLbvh, nullptr, g,
                           err) != hipSuccess)
      return fail(MRT_ERR_HIP, "device BVH build failed: " + err);
    s->nodes = std::move(g.nodes);
    s->tris = std::move(g.tris);
    b.build_ms = g.build_ms;
    // host copy of the tree for mrt_scene_check_bvh / info
    mrt::BvhResult& t = s->bvh;
    t.nodes.resize(s->nodes.bytes / 4);
    t.tris.resize(s->tris.bytes / 4);
    HIP_TRY(hipMemcpy(t.nodes.data(), s->nodes.p, s->nodes.bytes, hipMemcpyDeviceToHost));
    if (s->tris.bytes) HIP_TRY(hipMemcpy(t.tris.data(), s->tris.p, s->tris.bytes, hipMemcpyDeviceToHost));
    t.root = g.root;
    t.num_nodes = g.num_nodes;
    t.num_leaves = g.num_leaves;
    t.max_depth = g.levels;
    t.wide_depth = g.levels;
    t.width = 4;
    t.max_stack = g.max_stack;
    t.lds_nodes = std::min<uint32_t>(b.opt.lds_node_budget, g.num_nodes);   // BFS order: any prefix is the top
    t.sah_cost = 0.0;
  }
  if (s->bvh.max_stack > (uint32_t)mrt::kMaxTraversalStack)
    return fail(MRT_ERR_INVALID, "BVH needs a deeper traversal stack (" + std::to_string(s->bvh.max_stack) + " entries, " +
                                     std::to_string(s->bvh.wide_depth) + " levels)");
  return MRT_OK;
}

// stage 3: per-primitive shading records (primitive order), material and
// light records
void pack_records(SceneBuild& b) {
  const mrt::HostScene& h = b.s->host;
  b.prims.resize((size_t)b.T * 24);
  for (uint32_t t = 0; t < b.T; ++t) {
    const mrt::RefTriangleReference& r = h.references[t];
    float* o = &b.prims[(size_t)t * 24];
    for (int k = 0; k < 3; ++k) {
      const mrt::RefVertex& v = h.vertices[r.tri[k]];
      o[4 * k + 0] = v.v[0]; o[4 * k + 1] = v.v[1]; o[4 * k + 2] = v.v[2]; o[4 * k + 3] = 0.0f;
      o[12 + 4 * k + 0] = v.n[0]; o[12 + 4 * k + 1] = v.n[1]; o[12 + 4 * k + 2] = v.n[2]; o[12 + 4 * k + 3] = 0.0f;
    }
    o[3] = bitsf(r.materialIndex);
    o[7] = bitsf(r.lightTriangleIndex);
  }
  b.mats.resize(h.materials.size() * 8);
  for (size_t m = 0; m < h.materials.size(); ++m) {
    const mrt::RefMaterial& M = h.materials[m];
    float* o = &b.mats[m * 8];
    o[0] = M.diffuse[0]; o[1] = M.diffuse[1]; o[2] = M.diffuse[2]; o[3] = M.ior;
    o[4] = M.emissive[0]; o[5] = M.emissive[1]; o[6] = M.emissive[2]; o[7] = bitsf(M.materialType);
  }
  b.lights.assign(h.lights.size() * 28, 0.0f);
  for (size_t l = 0; l < h.lights.size(); ++l) {
    const mrt::RefLightTriangle& L = h.lights[l];
    float* o = &b.lights[l * 28];
    o[0] = L.emissive[0]; o[1] = L.emissive[1]; o[2] = L.emissive[2]; o[3] = L.area;
    const mrt::RefVertex* v[3] = {&L.v1, &L.v2, &L.v3};
    for (int k = 0; k < 3; ++k) {
      for (int c = 0; c < 3; ++c) { o[4 + 8 * k + c] = v[k]->v[c]; o[8 + 8 * k + c] = v[k]->n[c]; }
    }
    o[7] = L.pdf;
    o[11] = L.cdf;
    o[15] = bitsf(L.index);
  }
}

// stage 4: shadow-ray occluder tree (occluders.h): a second BVH4 over the
// triangles outside the culled supporting planes, appended to the main tree's
// node and leaf-triangle arrays (refs rebased); host-SAH scenes only
int build_occluder_tree(SceneBuild& b) {
  mrt_scene* s = b.s;
  const mrt::HostScene& h = s->host;
  const uint32_t T = b.T;
  mrt::OccluderSet& occ = b.occ;
  mrt::BvhResult& ob = b.ob;
  b.up_nodes = s->bvh.nodes;
  b.up_tris = s->bvh.tris;
  b.occ_on = b.builder == MRT_BVH_HOST_SAH && !b.desc->no_occluder_tree;
  if (const char* v = mrt::diag_env("MRT_OCCLUDERS")) b.occ_on = b.occ_on && std::atoi(v) != 0;
  if (b.occ_on) {
    std::vector<float> lv, ln;
    for (uint32_t l = 0; l < h.light_count; ++l)
      for (const mrt::RefVertex* v : {&h.lights[l].v1, &h.lights[l].v2, &h.lights[l].v3}) {
        lv.insert(lv.end(), {v->v[0], v->v[1], v->v[2]});
        ln.insert(ln.end(), {v->n[0], v->n[1], v->n[2]});
      }
    b.occ_on = mrt::find_occluders(h.vertices.data()->v, sizeof(mrt::RefVertex), (uint32_t)h.vertices.size(),
                                   h.indices.data(), T, lv.data(), ln.data(), h.light_count, occ);
  }
  // with few light triangles the occluder tree leaves them out: every shadow
  // ray enters the light's own leaf box, and the kernels test the other
  // light triangles in one wave-uniform loop instead (dev_shadow.h
  // lights_occlude; MRT_OCC_LIGHTS=0 keeps them in the tree)
  b.occ_lights = b.occ_on && h.light_count <= mrt::kOccLightsMax;
  if (const char* v = mrt::diag_env("MRT_OCC_LIGHTS")) b.occ_lights = b.occ_lights && std::atoi(v) != 0;
  if (b.occ_lights) {
    std::vector<uint8_t> is_light(T, 0);
    for (uint32_t l = 0; l < h.light_count; ++l)
      if (h.lights[l].index < T) is_light[h.lights[l].index] = 1;
    occ.keep.erase(std::remove_if(occ.keep.begin(), occ.keep.end(), [&](uint32_t t) { return is_light[t] != 0; }),
                   occ.keep.end());
  }
  if (!b.occ_on || occ.keep.empty()) return MRT_OK;
  const uint32_t node_base = (uint32_t)(s->bvh.nodes.size() / 32), tri_base = T;
  std::vector<uint32_t> sub;
  sub.reserve(occ.keep.size() * 3);
  for (uint32_t t : occ.keep) sub.insert(sub.end(), {h.indices[3 * t], h.indices[3 * t + 1], h.indices[3 * t + 2]});
  mrt::BvhBuildOptions oo = b.opt;
  oo.lds_node_budget = 0;
  if (const char* v = mrt::diag_env("MRT_OCC_LEAF"))
    oo.max_leaf_size = std::max(1u, std::min<uint32_t>(mrt::kMaxLeafSize, (uint32_t)std::strtoul(v, nullptr, 0)));
  if (const char* v = mrt::diag_env("MRT_OCC_TCOST")) oo.traversal_cost = std::strtof(v, nullptr);
  std::string err;
  if (!mrt::build_bvh(h.vertices.data()->v, sizeof(mrt::RefVertex), sub.data(), (uint32_t)occ.keep.size(), oo, ob, err))
    return fail(MRT_ERR_INVALID, "occluder BVH build failed: " + err);
  auto rebase = [&](int32_t r) -> int32_t {
    if (r == mrt::kEmptyChild) return r;
    if (r >= 0) return r + (int32_t)node_base;
    const uint32_t lr = ~(uint32_t)r;
    return mrt::leaf_ref((lr >> mrt::kLeafCountBits) + tri_base, (lr & (mrt::kMaxLeafSize - 1)) + 1);
  };
  for (uint32_t k = 0; k < ob.num_nodes; ++k)
    for (int c = 0; c < 4; ++c) {
      float& f = ob.nodes[32 * (size_t)k + 24 + c];
      f = bitsf((uint32_t)rebase((int32_t)fbits(f)));
    }
  for (size_t i = 0; i < occ.keep.size(); ++i) {   // leaf prim ids: subset position -> primitive
    float& f = ob.tris[12 * i + 3];
    f = bitsf(occ.keep[fbits(f)]);
  }
  // the renderer sizes its LDS stack by the deeper of the two trees
  // (dev.max_stack): an occluder tree deeper than the traversal stack
  // allows, or deeper than the main tree (it holds a subset of its
  // triangles, so it would only cost the main tree's stack variant), is
  // dropped and shadow rays traverse the main tree
  if (ob.max_stack > (uint32_t)mrt::kMaxTraversalStack || ob.max_stack > s->bvh.max_stack) {
    b.occ_on = false;
    return MRT_OK;
  }
  b.occ_root = rebase(ob.root);
  if (ob.num_nodes) b.up_nodes.insert(b.up_nodes.end(), ob.nodes.begin(), ob.nodes.begin() + 32 * (size_t)ob.num_nodes);
  b.up_tris.insert(b.up_tris.end(), ob.tris.begin(), ob.tris.end());
  s->occ_nodes.assign(ob.nodes.begin(), ob.nodes.begin() + 32 * (size_t)ob.num_nodes);
  s->occ_tris = ob.tris;
  s->occ_keep = occ.keep;
  s->occ_root = b.occ_root;
  s->occ_node_base = node_base;
  s->occ_max_stack = ob.max_stack;
  return MRT_OK;
}

// stage 5: convex occluders (occluders.h): every triangle of the light-free
// occluder tree on a convex solid; the solids' faces go to the kernels and
// each solid triangle's face index into its shading record (p2.w)
void find_convex_solids(SceneBuild& b) {
  const mrt::HostScene& h = b.s->host;
  const mrt::ConvexSet& conv = b.conv;
  b.conv_on = b.occ_on && b.occ_lights && b.occ_root != mrt::kEmptyChild;
  if (const char* v = mrt::diag_env("MRT_CONVEX")) b.conv_on = b.conv_on && std::atoi(v) != 0;
  if (b.conv_on)
    b.conv_on = mrt::find_convex_occluders(h.vertices.data()->v, sizeof(mrt::RefVertex), (uint32_t)h.vertices.size(),
                                           h.indices.data(), b.T, b.occ.keep, b.occ, b.conv);
  if (!b.conv_on) return;
  for (uint32_t t = 0; t < b.T; ++t) {
    const uint32_t code = conv.prim_face[t];   // c * 8 + face + 1, 0: not on a solid
    b.prims[(size_t)t * 24 + 11] = bitsf(code);
    // the face's outward unit normal in n0.w, n1.w, n2.w (dev_shadow.h convex_occlusion's own-face test)
    if (code)
      for (int c = 0; c < 3; ++c) b.prims[(size_t)t * 24 + 15 + 4 * c] = conv.face_normal[(code - 1) / 8][3 * ((code - 1) % 8) + c];
  }
}

// The nine counts of a DeviceScene that the staging mode is chosen by
// (path_preferred), for the probe below and for the scene's own struct.
// sweep_leaves: the records nearest queries would sweep (0: they walk)
void fill_counts(const SceneBuild& b, uint32_t sweep_leaves, mrt::DeviceScene& d) {
  const mrt_scene* s = b.s;
  d.num_nodes = s->bvh.num_nodes;
  d.num_triangles = b.T;
  d.num_materials = (uint32_t)s->host.materials.size();
  d.num_lights = s->host.light_count;
  d.lds_nodes = s->bvh.lds_nodes;
  d.width = s->bvh.width;
  d.occ_nodes = b.occ_on ? (uint32_t)(b.up_nodes.size() / 32) - s->bvh.num_nodes : 0u;   // (a leaf-root main tree keeps one dummy node)
  d.occ_tris = b.occ_on ? (uint32_t)b.occ.keep.size() : 0u;
  d.sweep_leaves = sweep_leaves;
}

// stage 6: leaf-box sweep: one record per leaf of the main tree, in node and
// slot order, with the child box as the parent node holds it.  Eligible: at most
// kSweepLeaves leaves under an interior root, and the scene still staged
// whole in LDS with the records added (MRT_SWEEP=0: the walk)
void build_sweep(SceneBuild& b) {
  mrt_scene* s = b.s;
  if (s->bvh.root >= 0 && s->bvh.num_leaves <= mrt::kSweepLeaves) {
    for (uint32_t k = 0; k < s->bvh.num_nodes; ++k) {
      const float* nd = &s->bvh.nodes[32 * (size_t)k];
      for (int c = 0; c < 4; ++c)
        if ((int32_t)fbits(nd[24 + c]) < 0)
          s->sweep_list.insert(s->sweep_list.end(), {nd[c], nd[8 + c], nd[16 + c], nd[24 + c],
                                                     nd[4 + c], nd[12 + c], nd[20 + c], 0.0f});
    }
  }
  // the kernels' list: triangle pairs (MRT_SWEEP_PAIRS=0: no two leaves share
  // a record); a non-default leaf size can push it over the cap: the scene walks
  bool pair_singles = true;
  if (const char* v = mrt::diag_env("MRT_SWEEP_PAIRS")) pair_singles = std::atoi(v) != 0;
  mrt::sweep_pair_records(s->sweep_list, pair_singles, s->sweep_pairs);
  b.sweep_leaves = (uint32_t)(s->sweep_pairs.size() / 8);
  if (b.sweep_leaves >= 1 && b.sweep_leaves <= mrt::kSweepLeaves && s->bvh.width == 4) {
    mrt::DeviceScene probe{};
    fill_counts(b, b.sweep_leaves, probe);
    s->sweep_on = !mrt::fast::path_preferred(probe);
  }
  if (const char* v = mrt::diag_env("MRT_SWEEP")) s->sweep_on = s->sweep_on && std::atoi(v) != 0;
  if (s->sweep_on) mrt::sweep_phase1_records(s->sweep_pairs, s->sweep_phase1);
  // rest pops per pass of the stream kernel's queue levels before a ray is
  // recycled (MRT_SWEEP_CAP: kSweepLeaves or more never recycles — the uncapped sweep)
  if (const char* v = mrt::diag_env("MRT_SWEEP_CAP"))
    s->sweep_cap = (uint32_t)std::min<unsigned long>(std::strtoul(v, nullptr, 0), mrt::kSweepLeaves);
}

// stage 7: mrt_scene_info (device_bytes: the upload's)
void fill_info(SceneBuild& b) {
  const mrt_scene* s = b.s;
  const mrt::HostScene& h = s->host;
  const mrt::OccluderSet& occ = b.occ;
  const mrt::ConvexSet& conv = b.conv;
  mrt_scene_info& in = b.s->info;
  if (b.conv_on) {
    in.convex_solids = conv.count;
    in.convex_delta = conv.delta;
    for (uint32_t c = 0; c < conv.count; ++c) {
      for (int i = 0; i < 16; ++i) in.convex_obb[c][i] = conv.obb[c][i];
      for (int k = 0; k < 8; ++k) in.convex_face_tris[c][k] = conv.face_tris[c][k];
    }
  }
  if (b.occ_on) {
    in.occluder_planes = (uint32_t)occ.planes.size();
    in.occluder_culled = occ.culled;
    in.occluder_nodes = b.ob.num_nodes;
    in.occluder_margin = occ.margin;
    in.occluder_max_stack = b.ob.max_stack;
    in.occluder_cos_min = occ.cos_min;
    for (size_t k = 0; k < occ.planes.size() && k < 8; ++k)
      for (int c = 0; c < 4; ++c) in.occluder_plane[k][c] = occ.planes[k][c];
  }
  in.vertices = (uint32_t)h.vertices.size();
  in.triangles = b.T;
  in.materials = (uint32_t)h.materials.size();
  in.light_triangles = h.light_count;
  in.bvh_nodes = s->bvh.num_nodes;
  in.bvh_leaves = s->bvh.num_leaves;
  in.bvh_depth = s->bvh.max_depth;
  in.bvh_lds_nodes = s->bvh.lds_nodes;
  in.bvh_width = s->bvh.width;
  in.bvh_max_stack = s->bvh.max_stack;
  in.bvh_sah_cost = s->bvh.sah_cost;
  in.build_ms = b.build_ms;
}

// stage 8: upload, and the DeviceScene the kernels get
int upload_scene(SceneBuild& b) {
  mrt_scene* s = b.s;
  const mrt::HostScene& h = s->host;
  const mrt::OccluderSet& occ = b.occ;
  const uint32_t T = b.T;
  // the kernels address nodes and leaf triangles with 32-bit buffer offsets
  // (dev_lds.h buf_ld4): each array below 4 GiB (~33 M nodes, ~89 M
  // triangles; a scene beyond that needs the flat-address build)
  if ((uint64_t)b.up_nodes.size() * 4 >= (1ull << 32) || (uint64_t)b.up_tris.size() * 4 >= (1ull << 32) ||
      (uint64_t)s->bvh.nodes.size() * 4 >= (1ull << 32) || (uint64_t)T * 48 >= (1ull << 32))
    return fail(MRT_ERR_INVALID, "scene too large: BVH nodes or leaf triangles exceed 4 GiB");
  HIP_TRY(hipSetDevice(b.desc->device));
  if (b.builder == MRT_BVH_HOST_SAH) {
    HIP_TRY(upload(s->nodes, b.up_nodes.data(), b.up_nodes.size() * 4));
    HIP_TRY(upload(s->tris, b.up_tris.data(), b.up_tris.size() * 4));
  }
  HIP_TRY(upload(s->prims, b.prims.data(), b.prims.size() * 4));
  HIP_TRY(upload(s->materials, b.mats.data(), b.mats.size() * 4));
  HIP_TRY(upload(s->lights, b.lights.data(), b.lights.size() * 4));
  mrt::DeviceScene& d = s->dev;
  d.nodes = s->nodes.as<float>();
  d.tris = s->tris.as<float>();
  d.prims = s->prims.as<float>();
  d.materials = s->materials.as<float>();
  d.lights = s->lights.as<float>();
  d.root = s->bvh.root;
  fill_counts(b, s->sweep_on ? b.sweep_leaves : 0u, d);
  d.max_stack = s->bvh.max_stack;
  d.origin_test = T >= mrt::kOriginTestTriangles ? 1u : 0u;   // (global-memory trees)
  if (const char* v = mrt::diag_env("MRT_ORIGIN_TEST")) d.origin_test = std::atoi(v) != 0;
  d.region_grabs = T >= mrt::kRegionGrabTriangles ? 1u : 0u;
  if (const char* v = mrt::diag_env("MRT_REGIONS")) d.region_grabs = std::atoi(v) != 0;
  d.light_shortcut = h.light_count <= mrt::kLightShortcutMax ? 1u : 0u;
  if (const char* v = mrt::diag_env("MRT_LAST_LIGHT")) d.light_shortcut = d.light_shortcut && std::atoi(v) != 0;
  d.occ_root = b.occ_root;
  d.occ_planes = 0;
  d.occ_lights = 0;
  if (b.occ_on) {
    d.occ_lights = b.occ_lights ? 1u : 0u;
    d.occ_planes = (uint32_t)occ.planes.size();
    d.occ_margin = occ.margin;
    d.occ_cos_min = occ.cos_min;
    d.occ_cos_min2 = occ.cos_min * occ.cos_min;
    for (uint32_t k = 0; k < d.occ_planes; ++k)
      for (int c = 0; c < 4; ++c) d.occ_plane[k][c] = occ.planes[k][c];
    d.max_stack = std::max(d.max_stack, b.ob.max_stack);
  }
  d.conv_count = s->info.convex_solids;
  std::memcpy(d.conv_obb, s->info.convex_obb, sizeof(d.conv_obb));
  std::memcpy(d.conv_face_tris, s->info.convex_face_tris, sizeof(d.conv_face_tris));
  d.sweep = nullptr;
  d.sweep_cap = s->sweep_cap;
  if (s->sweep_on) {
    // both lists in one buffer: the records, then at kSweepLeaves records phase 1's centre list
    std::vector<float> both(8 * (size_t)mrt::kSweepLeaves + s->sweep_phase1.size(), 0.0f);
    std::copy(s->sweep_pairs.begin(), s->sweep_pairs.end(), both.begin());
    std::copy(s->sweep_phase1.begin(), s->sweep_phase1.end(), both.begin() + 8 * (size_t)mrt::kSweepLeaves);
    HIP_TRY(upload(s->sweep, both.data(), both.size() * 4));
    d.sweep = s->sweep.as<float>();
  }
  HIP_TRY(alloc_isect_spill(s->isect_spill, d.max_stack));
  s->info.device_bytes = s->nodes.bytes + s->tris.bytes + s->prims.bytes + s->materials.bytes + s->lights.bytes +
                         s->sweep.bytes;
  return MRT_OK;
}

// Structural check of one BVH4 over the scene's primitives: every primitive
// in `want` in exactly one leaf (and no other), every child box contains its
// subtree's triangles, leaf records match the vertices, the stack bound
// holds.  node(ref) / tri(k) map the tree's (possibly rebased) references to
// host records; nodes [node_lo, node_lo + num_nodes) must all be reachable.
template <class NodeFn, class TriFn>
int check_tree(const mrt::HostScene& h, int32_t root, uint32_t node_lo, uint32_t num_nodes, uint32_t tri_lo,
               uint32_t tri_count, uint32_t max_stack, const std::vector<uint8_t>& want, NodeFn node, TriFn tri,
               const char* what) {
  const uint32_t T = (uint32_t)h.references.size();
  std::vector<uint8_t> seen(T, 0);
  auto fbits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
  auto bad = [&](const char* m) { return fail(MRT_ERR_STATE, std::string(what) + ": " + m); };
  // pend = stack entries pushed by the ancestors (bounded by max_stack)
  struct Item { int32_t ref; float lo[3], hi[3]; uint32_t depth, pend; };
  std::vector<Item> stack;
  stack.push_back(Item{root, {-1e30f, -1e30f, -1e30f}, {1e30f, 1e30f, 1e30f}, 0, 0});
  uint32_t nodes_seen = 0;
  while (!stack.empty()) {
    Item it = stack.back();
    stack.pop_back();
    if (it.depth >= (uint32_t)mrt::kMaxTraversalStack) return bad("BVH too deep");
    if (it.ref >= 0) {
      if ((uint32_t)it.ref < node_lo || (uint32_t)it.ref - node_lo >= num_nodes) return bad("BVH node index out of range");
      ++nodes_seen;
      Item ch[4];
      uint32_t nc = 0;
      {
        const float* n = node((uint32_t)it.ref);
        for (int c = 0; c < 4; ++c) {
          const int32_t ref = (int32_t)fbits(n[24 + c]);
          if (ref == mrt::kEmptyChild) continue;
          if (nc != (uint32_t)c) return bad("BVH4 empty slot before a used one");
          ch[nc++] = Item{ref, {n[c], n[8 + c], n[16 + c]}, {n[4 + c], n[12 + c], n[20 + c]}, it.depth + 1, 0};
        }
        if (nc < 2) return bad("BVH4 node with fewer than two children");
      }
      for (uint32_t c = 0; c < nc; ++c) {
        for (int k = 0; k < 3; ++k)
          if (!(ch[c].lo[k] <= ch[c].hi[k])) return bad("BVH empty child box");
        ch[c].pend = it.pend + nc - 1;
        if (ch[c].pend > max_stack) return bad("BVH stack bound too small");
        stack.push_back(ch[c]);
      }
    } else {
      const uint32_t leaf = ~(uint32_t)it.ref;
      const uint32_t first = leaf >> mrt::kLeafCountBits, cnt = (leaf & (mrt::kMaxLeafSize - 1)) + 1;
      if (first < tri_lo || first - tri_lo + cnt > tri_count) return bad("BVH leaf range out of bounds");
      for (uint32_t k = first; k < first + cnt; ++k) {
        const float* t = tri(k);
        const uint32_t prim = fbits(t[3]);
        if (prim >= T || !want[prim] || seen[prim]) return bad("BVH primitive missing, foreign or duplicated");
        seen[prim] = 1;
        for (int c = 0; c < 3; ++c) {
          const float* p = h.vertices[h.references[prim].tri[c]].v;
          for (int a = 0; a < 3; ++a)
            if (!(p[a] >= it.lo[a] && p[a] <= it.hi[a])) return bad("BVH box does not contain its triangle");
        }
        // leaf record = (v0, prim), (v1 - v0), (v2 - v0)
        const float* v0 = h.vertices[h.references[prim].tri[0]].v;
        const float* v1 = h.vertices[h.references[prim].tri[1]].v;
        const float* v2 = h.vertices[h.references[prim].tri[2]].v;
        for (int a = 0; a < 3; ++a)
          if (t[a] != v0[a] || t[4 + a] != v1[a] - v0[a] || t[8 + a] != v2[a] - v0[a])
            return bad("BVH leaf triangle record mismatch");
      }
    }
  }
  for (uint32_t t = 0; t < T; ++t)
    if (want[t] && !seen[t]) return bad("BVH primitive not referenced");
  if (nodes_seen != num_nodes) return bad("BVH has unreachable nodes");
  return MRT_OK;
}

// mrt_accel_create / _rebuild: the structure over the descriptor's buffers as they are now
int accel_build(mrt_accel* a) {
  const mrt_accel_desc& d = a->desc;
  const uint32_t T = d.triangle_count;
  const uint32_t leaf = d.max_leaf_size ? d.max_leaf_size : 2;
  HIP_TRY(hipSetDevice(d.device));
  hipStream_t s = (hipStream_t)d.stream;
  std::string err;
  if (a->info.builder != MRT_BVH_HOST_SAH) {
    mrt::GpuBvhResult g;
    if (mrt::build_bvh_gpu(reinterpret_cast<const float*>(d.vertices), d.vertex_stride, d.indices, T, leaf,
                           a->info.builder == MRT_BVH_DEVICE_PLOC ? mrt::GpuBvhAlgo::kPloc : mrt::GpuBvhAlgo::kLbvh,
                           s, g, err) != hipSuccess)
      return fail(MRT_ERR_HIP, "device BVH build failed: " + err);
    a->nodes = std::move(g.nodes);   // (a rebuild: the previous tree is freed)
    a->tris = std::move(g.tris);
    a->dev.root = g.root;
    a->dev.num_nodes = g.num_nodes;
    a->dev.max_stack = g.max_stack;
    a->info.bvh_nodes = g.num_nodes;
    a->info.bvh_leaves = g.num_leaves;
    a->info.bvh_levels = g.levels;
    a->info.bvh_max_stack = g.max_stack;
    a->info.build_ms = g.build_ms;
  } else {
    // host binned SAH: read the buffers back (the reference's own data path
    // never does this; kept for quality comparison and as a fallback-free
    // alternative for small scenes)
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t nv = 0;
    std::vector<uint32_t> idx((size_t)T * 3);
    if (T) HIP_TRY(hipMemcpy(idx.data(), d.indices, idx.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t v : idx) nv = std::max(nv, v + 1);
    std::vector<uint8_t> verts((size_t)nv * d.vertex_stride);
    if (nv) HIP_TRY(hipMemcpy(verts.data(), d.vertices, verts.size(), hipMemcpyDeviceToHost));
    mrt::BvhBuildOptions opt;
    opt.max_leaf_size = leaf;
    opt.width = 4;
    opt.lds_node_budget = 0;
    mrt::BvhResult b;
    const auto t0 = std::chrono::steady_clock::now();
    if (T == 0) return fail(MRT_ERR_INVALID, "host SAH build of an empty structure (use the device builder)");
    if (!mrt::build_bvh(reinterpret_cast<const float*>(verts.data()), d.vertex_stride, idx.data(), T, opt, b, err))
      return fail(MRT_ERR_INVALID, "BVH build failed: " + err);
    a->info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(upload(a->nodes, b.nodes.data(), b.nodes.size() * 4));
    HIP_TRY(upload(a->tris, b.tris.data(), b.tris.size() * 4));
    a->dev.root = b.root;
    a->dev.num_nodes = b.num_nodes;
    a->dev.max_stack = b.max_stack;
    a->info.bvh_nodes = b.num_nodes;
    a->info.bvh_leaves = b.num_leaves;
    a->info.bvh_levels = b.wide_depth;
    a->info.bvh_max_stack = b.max_stack;
  }
  if (a->dev.max_stack > (uint32_t)mrt::kMaxTraversalStack) return fail(MRT_ERR_INVALID, "BVH needs a deeper traversal stack");
  if ((uint64_t)a->nodes.bytes >= (1ull << 32) || (uint64_t)a->tris.bytes >= (1ull << 32))   // 32-bit buffer offsets
    return fail(MRT_ERR_INVALID, "acceleration structure too large: nodes or leaf triangles exceed 4 GiB");
  HIP_TRY(alloc_isect_spill(a->isect_spill, a->dev.max_stack));
  a->dev.nodes = a->nodes.as<float>();
  a->dev.tris = a->tris.as<float>();
  a->dev.num_triangles = T;
  a->dev.width = 4;
  a->dev.lds_nodes = 0;
  a->info.triangles = T;
  a->info.device_bytes = a->nodes.bytes + a->tris.bytes;
  return MRT_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// scene
// ---------------------------------------------------------------------------
int mrt_scene_create(const mrt_scene_desc* desc, mrt_scene** out) {
  if (!desc || !out || !desc->obj_path) return fail(MRT_ERR_INVALID, "mrt_scene_create: null argument");
  *out = nullptr;
  std::unique_ptr<mrt_scene> s(new mrt_scene());
  s->device = desc->device;
  std::string err;
  if (!mrt::import_obj(desc->obj_path, desc->mtl_override ? desc->mtl_override : "", s->host, err))
    return fail(MRT_ERR_IO, err);
  if (desc->procedural_triangles) mrt::append_procedural_mesh(s->host, desc->procedural_triangles, desc->procedural_seed);
  mrt::flatten(s->host);
  s->motion_digest = 14695981039346656037ull;
  for (const mrt::RefTriangleReference& t : s->host.references)
    for (const uint32_t w : {t.materialIndex, t.lightTriangleIndex == 0xFFFFFFFFu ? 0u : 1u})
      for (int k = 0; k < 4; ++k) s->motion_digest = (s->motion_digest ^ ((w >> (8 * k)) & 0xFFu)) * 1099511628211ull;
  SceneBuild b;
  b.desc = desc;
  b.s = s.get();
  b.T = (uint32_t)s->host.references.size();
  if (int rc = build_options(b)) return rc;
  if (int rc = build_main_tree(b)) return rc;
  pack_records(b);
  if (int rc = build_occluder_tree(b)) return rc;
  find_convex_solids(b);
  build_sweep(b);
  fill_info(b);
  // a host-only scene (CPU tests of import + BVH) ends here, before any HIP call
  if (desc->device >= 0)
    if (int rc = upload_scene(b)) return rc;
  *out = s.release();
  return MRT_OK;
}

int mrt_scene_info_get(const mrt_scene* scene, mrt_scene_info* info) {
  if (!scene || !info) return fail(MRT_ERR_INVALID, "null argument");
  *info = scene->info;
  return MRT_OK;
}

// host only.  O(1) for a compatible pair: equal counts and equal digests of what
// is compared (mrt_scene::motion_digest; two different sequences of a million
// words agree in 64 bits with probability 2^-64, and the kernels' reads stay
// inside both scenes' buffers whatever the words, since the counts are compared
// exactly).  Only a pair that differs is walked, to name the first difference
int mrt_scene_motion_compatible(const mrt_scene* a, const mrt_scene* b) {
  if (!a || !b) return fail(MRT_ERR_INVALID, "mrt_scene_motion_compatible: null argument");
  const auto& ra = a->host.references;
  const auto& rb = b->host.references;
  if (a == b || (ra.size() == rb.size() && a->host.materials.size() == b->host.materials.size() &&
                 a->motion_digest == b->motion_digest))
    return MRT_OK;
  if (ra.size() != rb.size())
    return fail(MRT_ERR_INVALID, "motion: the scenes have " + std::to_string(ra.size()) + " and " +
                                     std::to_string(rb.size()) + " triangles");
  if (a->host.materials.size() != b->host.materials.size())
    return fail(MRT_ERR_INVALID, "motion: the scenes have " + std::to_string(a->host.materials.size()) + " and " +
                                     std::to_string(b->host.materials.size()) + " materials");
  for (size_t k = 0; k < ra.size(); ++k) {
    if (ra[k].materialIndex != rb[k].materialIndex)
      return fail(MRT_ERR_INVALID, "motion: primitive " + std::to_string(k) + " has material " +
                                       std::to_string(ra[k].materialIndex) + " in one scene and " +
                                       std::to_string(rb[k].materialIndex) + " in the other");
    if ((ra[k].lightTriangleIndex == 0xFFFFFFFFu) != (rb[k].lightTriangleIndex == 0xFFFFFFFFu))
      return fail(MRT_ERR_INVALID, "motion: primitive " + std::to_string(k) + " is a light triangle in one scene only");
  }
  return MRT_OK;
}

int mrt_debug_sweep_list(const mrt_scene* scene, float* records, uint32_t capacity, uint32_t* count,
                         uint32_t* enabled) {
  if (!scene || !count || !enabled) return fail(MRT_ERR_INVALID, "mrt_debug_sweep_list: null argument");
  const uint32_t n = (uint32_t)(scene->sweep_list.size() / 8);
  if (records) std::memcpy(records, scene->sweep_list.data(), (size_t)std::min(n, capacity) * 32);
  *count = n;
  *enabled = scene->sweep_on ? 1u : 0u;
  return MRT_OK;
}

int mrt_debug_sweep_pairs(const mrt_scene* scene, float* records, uint32_t* prims, uint32_t capacity,
                          uint32_t* count) {
  if (!scene || !count) return fail(MRT_ERR_INVALID, "mrt_debug_sweep_pairs: null argument");
  const uint32_t n = (uint32_t)(scene->sweep_pairs.size() / 8), m = std::min(n, capacity);
  if (records) std::memcpy(records, scene->sweep_pairs.data(), (size_t)m * 32);
  if (prims)
    for (uint32_t i = 0; i < m; ++i) {
      const uint32_t w = fbits(scene->sweep_pairs[8 * (size_t)i + 3]);
      prims[2 * i] = fbits(scene->bvh.tris[12 * (size_t)(w & 0xFFFFu) + 3]);
      prims[2 * i + 1] = fbits(scene->bvh.tris[12 * (size_t)(w >> 16) + 3]);
    }
  *count = n;
  return MRT_OK;
}

int mrt_debug_sweep_phase1(const mrt_scene* scene, float* records, uint32_t capacity, uint32_t* count) {
  if (!scene || !count) return fail(MRT_ERR_INVALID, "mrt_debug_sweep_phase1: null argument");
  const uint32_t n = (uint32_t)(scene->sweep_phase1.size() / 8);
  if (records) std::memcpy(records, scene->sweep_phase1.data(), (size_t)std::min(n, capacity) * 32);
  *count = n;
  return MRT_OK;
}

int mrt_debug_sweep_cap(const mrt_scene* scene, uint32_t* cap) {
  if (!scene || !cap) return fail(MRT_ERR_INVALID, "mrt_debug_sweep_cap: null argument");
  *cap = scene->sweep_cap;
  return MRT_OK;
}

int mrt_debug_bvh_nodes(const mrt_scene* scene, float* nodes, uint32_t capacity, uint32_t* count) {
  if (!scene || !count) return fail(MRT_ERR_INVALID, "mrt_debug_bvh_nodes: null argument");
  const uint32_t n = scene->bvh.num_nodes;
  if (nodes) std::memcpy(nodes, scene->bvh.nodes.data(), (size_t)std::min(n, capacity) * 128);
  *count = n;
  return MRT_OK;
}

int mrt_scene_export(const mrt_scene* scene, void* vertices, void* indices, void* materials, void* references,
                     void* lights) {
  if (!scene) return fail(MRT_ERR_INVALID, "null scene");
  const mrt::HostScene& h = scene->host;
  if (vertices) std::memcpy(vertices, h.vertices.data(), h.vertices.size() * sizeof(mrt::RefVertex));
  if (indices) std::memcpy(indices, h.indices.data(), h.indices.size() * 4);
  if (materials) std::memcpy(materials, h.materials.data(), h.materials.size() * sizeof(mrt::RefMaterial));
  if (references) std::memcpy(references, h.references.data(), h.references.size() * sizeof(mrt::RefTriangleReference));
  if (lights) std::memcpy(lights, h.lights.data(), h.lights.size() * sizeof(mrt::RefLightTriangle));
  return MRT_OK;
}

int mrt_scene_check_bvh(const mrt_scene* scene) {
  if (!scene) return fail(MRT_ERR_INVALID, "null scene");
  const mrt::BvhResult& b = scene->bvh;
  const mrt::HostScene& h = scene->host;
  const uint32_t T = (uint32_t)h.references.size();
  std::vector<uint8_t> all(T, 1);
  if (const char* dn = mrt::diag_env("MRT_DUMP_NODE")) {   // diagnostic: one node's rows and its leaf triangles
    const uint32_t k = (uint32_t)std::strtoul(dn, nullptr, 0);
    if (k < b.num_nodes) {
      const float* n = &b.nodes[32 * (size_t)k];
      for (int i = 0; i < 32; ++i) std::fprintf(stderr, "NODE %u %d %08x %.9g\n", k, i, fbits(n[i]), n[i]);
      for (int c = 0; c < 4; ++c) {
        const int32_t r = (int32_t)fbits(n[24 + c]);
        if (r >= 0 || r == mrt::kEmptyChild) continue;
        const uint32_t lr = ~(uint32_t)r, first = lr >> mrt::kLeafCountBits, cnt = (lr & (mrt::kMaxLeafSize - 1)) + 1;
        for (uint32_t t = first; t < first + cnt; ++t)
          for (int i = 0; i < 12; ++i)
            std::fprintf(stderr, "TRI %d %u %d %08x\n", c, t, i, fbits(b.tris[12 * (size_t)t + i]));
      }
    }
  }
  int rc = check_tree(
      h, b.root, 0, b.num_nodes, 0, T, b.max_stack, all, [&](uint32_t r) { return &b.nodes[32 * (size_t)r]; },
      [&](uint32_t k) { return &b.tris[12 * (size_t)k]; }, "main tree");
  if (rc || scene->occ_keep.empty()) return rc;
  // the occluder tree: exactly the kept primitives, its own stack bound, which
  // the renderer's stack (sized by the deeper tree) covers
  std::vector<uint8_t> kept(T, 0);
  for (uint32_t p : scene->occ_keep) kept[p] = 1;
  const uint32_t occ_nodes = (uint32_t)(scene->occ_nodes.size() / 32);
  if (scene->occ_max_stack > b.max_stack) return fail(MRT_ERR_STATE, "occluder tree: deeper than the main tree");
  return check_tree(
      h, scene->occ_root, scene->occ_node_base, occ_nodes, T, (uint32_t)scene->occ_keep.size(), scene->occ_max_stack,
      kept, [&](uint32_t r) { return &scene->occ_nodes[32 * (size_t)(r - scene->occ_node_base)]; },
      [&](uint32_t k) { return &scene->occ_tris[12 * (size_t)(k - T)]; }, "occluder tree");
}

int mrt_debug_box_margin(const mrt_scene* scene, const void* rays, uint32_t stride, uint32_t count,
                         const void* intersections, float* out) {
  if (!scene || (count && (!rays || !intersections || !out))) return fail(MRT_ERR_INVALID, "null argument");
  if (stride < 32 || stride % 4) return fail(MRT_ERR_INVALID, "ray stride must be >= 32 and a multiple of 4");
  const mrt::BvhResult& b = scene->bvh;
  const mrt::HostScene& h = scene->host;
  const uint32_t T = (uint32_t)h.references.size();
  // (parent node, child slot) of every interior node and of every primitive's leaf
  struct Up { uint32_t node, slot; };
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  std::vector<Up> node_up(b.num_nodes, Up{kNone, 0}), prim_up(T, Up{kNone, 0});
  if (b.root >= 0)
    for (uint32_t n = 0; n < b.num_nodes; ++n)
      for (uint32_t c = 0; c < 4; ++c) {
        const int32_t ref = (int32_t)fbits(b.nodes[32 * (size_t)n + 24 + c]);
        if (ref == mrt::kEmptyChild) continue;
        if (ref >= 0) { node_up[ref] = Up{n, c}; continue; }
        const uint32_t lr = ~(uint32_t)ref, first = lr >> mrt::kLeafCountBits, cnt = (lr & (mrt::kMaxLeafSize - 1)) + 1;
        for (uint32_t k = first; k < first + cnt; ++k) prim_up[fbits(b.tris[12 * (size_t)k + 3])] = Up{n, c};
      }
  // triangles around each vertex position (vertex records are per (position,
  // normal), so corners are matched by their position bits)
  std::vector<std::pair<uint64_t, uint32_t>> corner;   // (hash of position, triangle)
  corner.reserve(3 * (size_t)T);
  auto pos_key = [&](uint32_t vi) {
    const float* v = h.vertices[vi].v;
    return ((uint64_t)fbits(v[0]) * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)fbits(v[1]) * 0xC2B2AE3D27D4EB4Full) ^
           ((uint64_t)fbits(v[2]) * 0x165667B19E3779F9ull);
  };
  for (uint32_t t = 0; t < T; ++t)
    for (int c = 0; c < 3; ++c) corner.emplace_back(pos_key(h.references[t].tri[c]), t);
  std::sort(corner.begin(), corner.end());
  const uint8_t* rp = static_cast<const uint8_t*>(rays);
  const mrt::RefIntersection* is = static_cast<const mrt::RefIntersection*>(intersections);
  for (uint32_t i = 0; i < count; ++i) {
    const float* f = reinterpret_cast<const float*>(rp + (size_t)i * stride);
    float* o4 = out + 4 * (size_t)i;
    o4[0] = o4[1] = o4[2] = o4[3] = -INFINITY;   // a miss, or a leaf-root tree (no box above the triangle)
    if (!(is[i].distance >= 0.0f) || is[i].triangleIndex >= T || prim_up[is[i].triangleIndex].node == kNone) continue;
    const float tmin = f[3];
    float inv[3], oinv[3];
    for (int a = 0; a < 3; ++a) {   // dev_math.h make_raybox (the fast build's reciprocal correctly rounded here)
      const float d = f[4 + a], dd = std::fabs(d) > 1e-20f ? d : std::copysign(1e-20f, d);
      inv[a] = 1.0f / dd;
      oinv[a] = f[a] * inv[a];
    }
    // the worst (t_entry - t) / t over the boxes above primitive k's leaf
    auto margin = [&](uint32_t k, float t, float* worst) {
      for (Up u = prim_up[k]; u.node != kNone; u = node_up[u.node]) {
        const float* n = &b.nodes[32 * (size_t)u.node];
        for (int form = 0; form < 2; ++form) {   // 0: precise (p - o) * inv, 1: fast fma(p, inv, -o * inv)
          float tn = tmin, tf = INFINITY;
          for (int a = 0; a < 3; ++a) {
            const float lo = n[8 * a + u.slot], hi = n[8 * a + 4 + u.slot];
            const float x0 = form ? std::fma(lo, inv[a], -oinv[a]) : (lo - f[a]) * inv[a];
            const float x1 = form ? std::fma(hi, inv[a], -oinv[a]) : (hi - f[a]) * inv[a];
            tn = std::fmax(tn, std::fmin(x0, x1));
            tf = std::fmin(tf, std::fmax(x0, x1));
          }
          // a box the ray's slab interval misses altogether: no culling slack finds the triangle
          worst[form] = std::fmax(worst[form], tn <= tf ? (tn - t) / t : INFINITY);
        }
      }
    };
    const uint32_t hit = is[i].triangleIndex;
    const float t_hit = is[i].distance;
    margin(hit, t_hit, o4);
    // near ties: triangles sharing a vertex position with the hit whose
    // Moller-Trumbore test some rounding of its float operations could pass
    // (a build that rounds differently — FMA contraction, an approximate
    // reciprocal — may report one of them instead, at its own t: DESIGN.md
    // §3.1's ray).  b1, b2 and t are evaluated exactly (double, on the float
    // inputs) with first-order error bounds of 4u per operation chain; a
    // neighbour counts when every test passes within its bound, and its slack
    // is taken at the smallest t the bound allows.
    const double o[3] = {f[0], f[1], f[2]}, d[3] = {f[4], f[5], f[6]};
    std::vector<uint32_t> ring;
    for (int c = 0; c < 3; ++c) {
      const uint64_t key = pos_key(h.references[hit].tri[c]);
      for (auto it = std::lower_bound(corner.begin(), corner.end(), std::make_pair(key, 0u));
           it != corner.end() && it->first == key; ++it)
        if (it->second != hit) ring.push_back(it->second);
    }
    std::sort(ring.begin(), ring.end());
    ring.erase(std::unique(ring.begin(), ring.end()), ring.end());
    auto norm = [](const double* x) { return std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); };
    for (uint32_t k : ring) {
      const float* v0 = h.vertices[h.references[k].tri[0]].v;
      const float* v1 = h.vertices[h.references[k].tri[1]].v;
      const float* v2 = h.vertices[h.references[k].tri[2]].v;
      double e1[3], e2[3], sv[3];   // e1, e2 as the kernels' float records hold them
      for (int a = 0; a < 3; ++a) {
        e1[a] = (double)(v1[a] - v0[a]);
        e2[a] = (double)(v2[a] - v0[a]);
        sv[a] = o[a] - (double)v0[a];
      }
      const double p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
      const double q[3] = {sv[1] * e1[2] - sv[2] * e1[1], sv[2] * e1[0] - sv[0] * e1[2], sv[0] * e1[1] - sv[1] * e1[0]};
      const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
      if (det == 0.0) continue;
      const double b1 = (sv[0] * p[0] + sv[1] * p[1] + sv[2] * p[2]) / det;
      const double b2 = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) / det;
      const double t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
      constexpr double u4 = 4.0 * 0x1p-24;
      const double np = norm(p), nq = norm(sv) * norm(e1) + norm(q), ad = std::fabs(det);
      const double eb1 = u4 * (norm(sv) * np + std::fabs(b1) * norm(e1) * np) / ad;
      const double eb2 = u4 * (norm(d) * nq + std::fabs(b2) * norm(e1) * np) / ad;
      const double et = u4 * (norm(e2) * nq + std::fabs(t) * norm(e1) * np) / ad;
      if (!(b1 >= -eb1 && b2 >= -eb2 && b1 + b2 <= 1.0 + eb1 + eb2 && t + et >= tmin && t - et > 0.0)) continue;
      if (!(std::fabs(t - t_hit) <= 0x1p-10 * t_hit + et)) continue;
      margin(k, (float)(t - et), o4 + 2);
    }
  }
  return MRT_OK;
}

int mrt_scene_destroy(mrt_scene* scene) {
  delete scene;
  return MRT_OK;
}

// ---------------------------------------------------------------------------
// acceleration structure over raw buffers (MPSTriangleAccelerationStructure +
// MPSRayIntersector, renderer/Renderer.mm:456-469)
// ---------------------------------------------------------------------------
int mrt_accel_create(const mrt_accel_desc* desc, mrt_accel** out) {
  if (!desc || !out) return fail(MRT_ERR_INVALID, "mrt_accel_create: null argument");
  *out = nullptr;
  if (desc->triangle_count && (!desc->vertices || !desc->indices))
    return fail(MRT_ERR_INVALID, "mrt_accel_create: null buffer");
  if (desc->vertex_stride < 12 || desc->vertex_stride % 4) return fail(MRT_ERR_INVALID, "mrt_accel_create: bad vertex_stride");
  if (desc->max_leaf_size > (uint32_t)mrt::kMaxLeafSize) return fail(MRT_ERR_INVALID, "mrt_accel_create: max_leaf_size > 16");
  const uint32_t builder = desc->builder ? desc->builder : MRT_BVH_DEVICE_PLOC;
  if (builder != MRT_BVH_HOST_SAH && builder != MRT_BVH_DEVICE_LBVH && builder != MRT_BVH_DEVICE_PLOC)
    return fail(MRT_ERR_INVALID, "unknown builder");
  std::unique_ptr<mrt_accel> a(new mrt_accel());
  a->desc = *desc;
  a->info.builder = builder;
  const int rc = accel_build(a.get());
  if (rc) return rc;
  *out = a.release();
  return MRT_OK;
}

int mrt_accel_rebuild(mrt_accel* accel) {
  if (!accel) return fail(MRT_ERR_INVALID, "null accel");
  return accel_build(accel);
}

int mrt_accel_intersect(const mrt_accel* accel, const void* rays, uint32_t stride, uint32_t count, void* isect,
                        uint32_t flags, void* stream) {
  if (!accel || (!rays && count) || (!isect && count) || stride < 32 || (stride % 4))
    return fail(MRT_ERR_INVALID, "mrt_accel_intersect: bad argument");
  HIP_TRY(hipSetDevice(accel->desc.device));
  HIP_TRY(MRT_BUILD_CALL(flags, launch_intersect(accel->dev, rays, stride, count, (mrt::RefIntersection*)isect,
                                                 accel->isect_spill.as<uint32_t>(), (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_accel_info_get(const mrt_accel* accel, mrt_accel_info* info) {
  if (!accel || !info) return fail(MRT_ERR_INVALID, "null argument");
  *info = accel->info;
  return MRT_OK;
}

int mrt_accel_destroy(mrt_accel* accel) {
  delete accel;
  return MRT_OK;
}

}  // extern "C"
