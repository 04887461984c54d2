// libislpose runtime: network graphs, weight upload (the packs are built in pack.cpp),
// activation arena and the C ABI of include/islpose.h.
//
// The three networks of src/model.py are rebuilt here as static graphs over
// padded buffers in 8-channel chunks.  Every torch.cat of the reference (model.py:177, 190,
// 199, 308-324, 397-405) becomes a channel-slice layout decision: producers
// write their slice of a shared buffer, consumers read the whole span, and the
// conv weights are repacked so that logical input channel order (the concat
// order of the reference) maps onto the physical slices.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>


#include "internal.h"
#include "islpose.h"
#include "pack.h"

namespace isl {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

static int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

#define HIP_OK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      std::string m_ = g_err.empty() ? "" : (" (" + g_err + ")");                     \
      return fail(ISL_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + m_); \
    }                                                                                 \
  } while (0)

// ---------------------------------------------------------------------------
// layer tables (model.py)
// ---------------------------------------------------------------------------

static_assert(PACK_ACT_PRELU == ACT_PRELU && PACK_WINO_X3_BCO == WINO_X3_BCO, "pack.h mirrors internal.h");

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// A layer: its host view (pack.h) and its device buffers, all owned here and freed in
// isl_net_destroy
struct ConvLayer : PackLayer {
  std::string name, prelu;
  bool has_w = false, has_b = false, has_s = false;
  // the packs the layer owns (owns_pack), [kind][full | hi-only].  The hi-only forms are
  // ISL_PREC_FP16's: the same 2^s, the same layouts without [hi|lo], built when the mode is
  // first used (upload_hi_packs)
  DevBuf dev[PK_COUNT][2];
  float inv[PK_COUNT];           // 2^-s of the split packs
  DevBuf par[PB_COUNT];          // bias and slopes, padded (build_param)
  ConvLayer() { std::fill(inv, inv + PK_COUNT, 1.f); }
  const void* pack(int kind, bool h16 = false) const { return dev[kind][h16].p; }
  const float* param(int which) const { return (const float*)par[which].p; }
  // Mconv6 of the fused pair: one tile of all its channels, which is PK_X3 where bco == cout
  int pair6_kind() const { return owns_pack(*this, PK_X3F) ? PK_X3F : PK_X3; }
};

static ConvLayer mk(const std::string& name, int cin, int cout, int k, int act, const std::string& prelu = "") {
  ConvLayer c;
  c.name = name; c.cin = cin; c.cout = cout; c.k = k; c.act = act; c.prelu = prelu;
  return c;
}

static void vgg_front(std::vector<ConvLayer>& L, bool hand, const std::vector<std::string>& prelu) {
  struct { const char* n; int ci, co; } t[] = {
      {"conv1_1", 3, 64},    {"conv1_2", 64, 64},   {"conv2_1", 64, 128},  {"conv2_2", 128, 128},
      {"conv3_1", 128, 256}, {"conv3_2", 256, 256}, {"conv3_3", 256, 256}, {"conv3_4", 256, 256},
      {"conv4_1", 256, 512}, {"conv4_2", 512, 512}};
  for (auto& e : t) {
    const bool p = std::find(prelu.begin(), prelu.end(), e.n) != prelu.end();
    // make_layers: PReLU named 'prelu' + name[4:] (model.py:43)
    L.push_back(mk(e.n, e.ci, e.co, 3, p ? ACT_PRELU : ACT_RELU, p ? "prelu" + std::string(e.n + 4) : ""));
  }
  if (hand) {
    L.push_back(mk("conv4_3", 512, 512, 3, ACT_RELU));
    L.push_back(mk("conv4_4", 512, 512, 3, ACT_RELU));
    L.push_back(mk("conv5_1", 512, 512, 3, ACT_RELU));
    L.push_back(mk("conv5_2", 512, 512, 3, ACT_RELU));
    L.push_back(mk("conv5_3_CPM", 512, 128, 3, ACT_RELU));
  } else {
    for (auto n : {"conv4_3_CPM", "conv4_4_CPM"}) {
      const bool p = std::find(prelu.begin(), prelu.end(), n) != prelu.end();
      const int ci = std::string(n) == "conv4_3_CPM" ? 512 : 256, co = ci == 512 ? 256 : 128;
      L.push_back(mk(n, ci, co, 3, p ? ACT_PRELU : ACT_RELU, p ? "prelu" + std::string(n + 4) : ""));
    }
  }
}

static std::vector<ConvLayer> body25_layers() {  // model.py:66-165
  std::vector<ConvLayer> L;
  vgg_front(L, false, {"conv4_2", "conv4_3_CPM", "conv4_4_CPM"});
  const std::vector<std::string> no_act = {"Mconv7_stage0_L1", "Mconv7_stage0_L2", "Mconv7_stage1_L1",
                                           "Mconv7_stage1_L2", "Mconv7_stage2_L2", "Mconv7_stage3_L2"};
  auto mc = [&](const std::string& n, int ci, int co, int k) {
    const bool none = std::find(no_act.begin(), no_act.end(), n) != no_act.end();
    // make_layers_Mconv: PReLU 'Mprelu' + name[5:] (model.py:61-62)
    L.push_back(mk(n, ci, co, k, none ? ACT_NONE : ACT_PRELU, none ? "" : "Mprelu" + n.substr(5)));
  };
  auto stage = [&](const std::string& tag, int cin, int w, int c6, int cout) {
    for (int b = 1; b <= 5; ++b)
      for (int j = 0; j < 3; ++j)
        mc("Mconv" + std::to_string(b) + "_" + tag + "_" + std::to_string(j), j ? w : (b == 1 ? cin : 3 * w), w, 3);
    mc("Mconv6_" + tag, 3 * w, c6, 1);
    mc("Mconv7_" + tag, c6, cout, 1);
  };
  stage("stage0_L2", 128, 96, 256, 52);
  for (int s = 1; s < 4; ++s) stage("stage" + std::to_string(s) + "_L2", 180, 128, 512, 52);
  stage("stage0_L1", 180, 96, 256, 26);
  stage("stage1_L1", 206, 128, 512, 26);
  return L;
}

static std::vector<ConvLayer> coco_layers() {  // model.py:210-299
  std::vector<ConvLayer> L;
  vgg_front(L, false, {});
  // model.py:215-218: 'Mconv7_stage6_L1' listed twice, 'Mconv7_stage6_L2' never -> keeps its ReLU
  auto none = [](const std::string& n) {
    if (n == "conv5_5_CPM_L1" || n == "conv5_5_CPM_L2" || n == "Mconv7_stage6_L1") return true;
    for (int i = 2; i <= 5; ++i)
      for (int b = 1; b <= 2; ++b)
        if (n == "Mconv7_stage" + std::to_string(i) + "_L" + std::to_string(b)) return true;
    return false;
  };
  auto c = [&](const std::string& n, int ci, int co, int k) { L.push_back(mk(n, ci, co, k, none(n) ? ACT_NONE : ACT_RELU)); };
  for (int br = 1; br <= 2; ++br) {
    const std::string s = "_L" + std::to_string(br);
    c("conv5_1_CPM" + s, 128, 128, 3); c("conv5_2_CPM" + s, 128, 128, 3); c("conv5_3_CPM" + s, 128, 128, 3);
    c("conv5_4_CPM" + s, 128, 512, 1); c("conv5_5_CPM" + s, 512, br == 1 ? 38 : 19, 1);
  }
  for (int i = 2; i <= 6; ++i)
    for (int br = 1; br <= 2; ++br) {
      const std::string s = "_stage" + std::to_string(i) + "_L" + std::to_string(br);
      c("Mconv1" + s, 185, 128, 7);
      for (int j = 2; j <= 5; ++j) c("Mconv" + std::to_string(j) + s, 128, 128, 7);
      c("Mconv6" + s, 128, 128, 1);
      c("Mconv7" + s, 128, br == 1 ? 38 : 19, 1);
    }
  return L;
}

static std::vector<ConvLayer> hand_layers() {  // model.py:331-392
  std::vector<ConvLayer> L;
  vgg_front(L, true, {});
  L.push_back(mk("conv6_1_CPM", 128, 512, 1, ACT_RELU));
  L.push_back(mk("conv6_2_CPM", 512, 22, 1, ACT_NONE));
  for (int i = 2; i <= 6; ++i) {
    const std::string s = "_stage" + std::to_string(i);
    L.push_back(mk("Mconv1" + s, 150, 128, 7, ACT_RELU));
    for (int j = 2; j <= 5; ++j) L.push_back(mk("Mconv" + std::to_string(j) + s, 128, 128, 7, ACT_RELU));
    L.push_back(mk("Mconv6" + s, 128, 128, 1, ACT_RELU));
    L.push_back(mk("Mconv7" + s, 128, 22, 1, ACT_NONE));
  }
  return L;
}

// ---------------------------------------------------------------------------
// graph
// ---------------------------------------------------------------------------

struct BufSpec {
  int level, cs, pad;
  int half = 0;   // W/2 wide (the pair-max buffer of a fused pool, ConvLaunch::hpool)
  int out32 = 0;  // the fp32 copy of a net output in an fp16-storage arena (no bytes in an fp32 arena)
};

struct Op {
  int type;  // 0 conv, 1 maxpool
  int layer;
  int in, in_coff, out, out_coff, C;
  int hbuf = -1;  // maxpool: the pair-max buffer its producing conv may write instead of `in`
  bool fuse67 = false;   // conv: this op and the next run as one fused 1x1 pair (plan_fuse67)
};

struct OutRef {
  int buf, coff, C;
};

}  // namespace isl

using namespace isl;

struct isl_net {
  int kind = 0, device = 0;
  std::vector<ConvLayer> layers;
  std::map<std::string, int> layer_index;
  std::vector<std::pair<std::string, int64_t>> params;  // caffe name, numel
  std::vector<BufSpec> bufs;
  std::vector<Op> ops;
  int in_buf = 0;
  OutRef out0{}, out1{};
  int n_out = 2;
  // ISL_ACT_FP16: per net output, its fp32 buffer in an fp16-storage arena (channels from 0)
  // and the op that writes the output last (its epilogue stores both)
  int out32_buf[2] = {-1, -1}, out_op[2] = {-1, -1};
  bool packed = false;
  bool packed_hi = false;      // the hi-only packs (ISL_PREC_FP16) match the current weights
  // plan
  int pn = 0, ph = 0, pw = 0;
  std::vector<Act> act;
  // activation arenas by net input size (h, w), sized by frame capacity (plan())
  struct Arena {
    void* base = nullptr;
    bool a16 = false;           // an fp16-storage arena (ISL_ACT_FP16): Act::esize 2 between the convs
    int n_cap = 0;
    std::vector<size_t> offs;   // buffer offsets for n_cap frames
    size_t bytes = 0;
    unsigned long long last_use = 0;
    // per-arena (per net size) pre-processing table and split-K workspace, so runs of
    // different sizes may be in flight on different streams at once (the hand scales)
    void* tab = nullptr;
    size_t tab_bytes = 0;
    std::vector<char> tab_host;   // what `tab` holds (upload_tab skips an identical table)
    // pinned staging of the table upload (a pageable hipMemcpyAsync may block the host until
    // the stream reaches it) and the event behind the copy out of it
    void* tab_pin = nullptr;
    size_t tab_pin_bytes = 0;
    hipEvent_t tab_ev = nullptr;
    float* ks = nullptr;
    size_t ks_floats = 0;
    // split-K fold plan for the current batch size (plan_fold): per op, the offset of a
    // producer's partial sums in fold_mem (-1: none) and of a consumer's X3Fold table in
    // fold_tab (-1: none)
    int fold_n = -1, fold_mode = -1;
    std::vector<long long> fold_ws_off, fold_tab_off;
    float* fold_mem = nullptr;
    size_t fold_mem_floats = 0;
    X3Fold* fold_tab = nullptr;
    size_t fold_tab_n = 0;
    // the conv chain replayed as a HIP graph (run_ops): per run key (batch, K-range mode,
    // algorithm, ISLPOSE_* environment) the eager runs seen and the instantiated graph
    struct Graph {
      hipGraphExec_t exec = nullptr;
      hipEvent_t done = nullptr;     // recorded behind its latest replay, on the replay's stream
      std::vector<int> op_variant;
      unsigned long long last_use = 0;
    };
    std::map<unsigned long long, Graph> graphs;
    unsigned long long graph_clock = 0;
    std::map<unsigned long long, int> graph_seen;
    std::set<unsigned long long> graph_failed;   // keys whose capture failed: eager for good
    std::vector<Graph> graph_retired;            // evicted, freed once their `done` has passed
  };
  std::map<long long, Arena> plans;
  Arena* cur = nullptr;        // the arena of the current plan
  unsigned long long plan_clock = 0;
  size_t plans_bytes = 0;
  void* arena = nullptr;
  // post scratch
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  PostLanes* lanes = nullptr;   // isl_hand_post_crops (net_post_lanes)
  // per-op event timing (isl_net_set_timing / isl_net_timing)
  struct TimedRun {
    std::vector<hipEvent_t> ev;          // ops + 1 events: before op 0, after every op
    std::vector<int> kind;
    std::vector<double> flops, mfma_flops;
  };
  bool timing = false;
  std::vector<TimedRun> timed;
  std::vector<int> op_variant;   // per op of the last run: x3_variant_code, -1 pool skipped (vin), 0 other
  // graph replay of the conv chain (isl_net_set_graph; off by default: measured level at batch 32
  // and 2.5 % slower at batch 1 in round 4, profiles/r04/r4v; env ISLPOSE_NET_GRAPH=0|1 overrides)
  int graph = 0;
  bool capturing = false;
  hipStream_t cap_stream = nullptr;
  // conv algorithm (ISL_ALGO_*) and the split-fp16 range flag (isl_net_check)
  int algo = ISL_ALGO_X3;
  // ISL_PREC_*: products per MAC of the ISL_ALGO_X3 convs (isl_net_set_precision, env
  // ISLPOSE_PRECISION=fp32|fp16); stored without effect under the other algorithms
  int precision = ISL_PREC_FP32;
  // ISL_ACT_*: storage of the activations between the ISL_PREC_FP16 convs (isl_net_set_act_storage,
  // env ISLPOSE_ACT_STORAGE=fp32|fp16); stored without effect otherwise.  a16_active: the arena
  // of the current plan is an fp16-storage one (plan() decides, per run, all or nothing)
  int act_storage = ISL_ACT_FP32;
  bool a16_active = false;
  int split_k = 1;             // isl_net_set_split_k: K-range mode (env ISLPOSE_X3_SPLITK=0|1|2)
  int* d_flag = nullptr;
  // range-guard trips: seen by the synchronous check (host count) and by the stream-ordered
  // one (device count, range_count_kernel); isl_net_range_info sums them
  long long range_trips_host = 0;
  unsigned long long* d_trips = nullptr;
  // per caller stream, an event recorded behind the latest work that writes d_flag / d_trips
  // there (run_ops, isl_net_check_async): the synchronous check and isl_net_range_info wait for
  // these instead of draining the device; owned events, so a stream the caller
  // has destroyed since is no hazard
  std::map<hipStream_t, hipEvent_t> flag_events;
  // pre-processing image table (host staging; the device copy is per arena)
  void* d_tab = nullptr;       // the current arena's table (Arena::tab)
  std::vector<char> h_tab;
};

namespace isl {

static int round8(int c) { return (c + 7) / 8 * 8; }

struct Builder {
  isl_net* net;
  int buf(int level, int cs, int pad, int half = 0) {
    net->bufs.push_back({level, cs, pad, half});
    return (int)net->bufs.size() - 1;
  }
  int L(const std::string& name) {
    auto it = net->layer_index.find(name);
    if (it == net->layer_index.end()) {
      fprintf(stderr, "islpose: graph references unknown layer %s\n", name.c_str());
      abort();
    }
    return it->second;
  }
  // conv reading logical channels through `cmap` (relative to in_coff)
  void conv(const std::string& name, int in, int in_coff, int out, int out_coff, std::vector<Seg> cmap = {},
            int cin_phys = 0) {
    const int li = L(name);
    ConvLayer& c = net->layers[li];
    if (cmap.empty()) cmap = {{0, 0, c.cin}};
    if (!cin_phys) cin_phys = round8(c.cin);
    c.cmap = cmap;
    c.cin_phys = cin_phys;
    c.bco = conv_bco_for(c.cout);
    c.x3_wide = x3_wide1_layer(c.k, c.cout, c.cin_phys);
    c.wbco = c.k == 3 ? wino_bco_for(c.cout) : 0;
    net->ops.push_back({0, li, in, in_coff, out, out_coff, 0});
  }
  // 2x2 max-pool of `in` (channels [0, C)) into `out`; when the producing conv can (x3,
  // even width) it writes pair maxima into a separate half-width buffer instead and
  // the pool takes the row pairs (run_ops)
  void pool(int in, int out, int C) {
    const int hb = buf(net->bufs[in].level, net->bufs[in].cs, 0, 1);
    net->ops.push_back({1, -1, in, 0, out, 0, C, hb});
  }

  // shared VGG front; returns the level-3 buffer written by the last front conv
  void front(int X, bool hand, int out_buf, int out_coff, int pad3) {
    int A1 = buf(0, 64, 1), A2 = buf(0, 64, 1), B1 = buf(1, 64, 1), B2 = buf(1, 128, 1), B3 = buf(1, 128, 1);
    int C1 = buf(2, 128, 1), C2 = buf(2, 256, 1), C3 = buf(2, 256, 1);
    int D1 = buf(3, 256, 1), D2 = buf(3, 512, 1), D3 = buf(3, 512, 1);
    (void)pad3;
    conv("conv1_1", X, 0, A1, 0);
    conv("conv1_2", A1, 0, A2, 0);
    pool(A2, B1, 64);
    conv("conv2_1", B1, 0, B2, 0);
    conv("conv2_2", B2, 0, B3, 0);
    pool(B3, C1, 128);
    conv("conv3_1", C1, 0, C2, 0);
    conv("conv3_2", C2, 0, C3, 0);
    conv("conv3_3", C3, 0, C2, 0);
    conv("conv3_4", C2, 0, C3, 0);
    pool(C3, D1, 256);
    conv("conv4_1", D1, 0, D2, 0);
    conv("conv4_2", D2, 0, D3, 0);
    if (hand) {
      conv("conv4_3", D3, 0, D2, 0);
      conv("conv4_4", D2, 0, D3, 0);
      conv("conv5_1", D3, 0, D2, 0);
      conv("conv5_2", D2, 0, D3, 0);
      conv("conv5_3_CPM", D3, 0, out_buf, out_coff);
    } else {
      conv("conv4_3_CPM", D3, 0, D2, 0);
      conv("conv4_4_CPM", D2, 0, out_buf, out_coff);
    }
  }
};

static void build_body25(isl_net* net) {
  Builder b{net};
  const int X = b.buf(0, 8, 1);
  net->in_buf = X;
  // stage input: [out0 0:128 | paf 128:180 (gap to 184) | heat0 184:210 (gap to 216)]
  const int SIN = b.buf(3, 216, 1), CA = b.buf(3, 384, 1), CB = b.buf(3, 384, 1), T6 = b.buf(3, 512, 1);
  const int HOUT = b.buf(3, 32, 1);
  b.front(X, false, SIN, 0, 1);
  auto stage = [&](const std::string& tag, int w, std::vector<Seg> cmap, int cin_phys, int out, int out_coff) {
    int cur = CA, oth = CB;
    for (int j = 0; j < 3; ++j)
      b.conv("Mconv1_" + tag + "_" + std::to_string(j), j ? cur : SIN, j ? (j - 1) * w : 0, cur, j * w,
             j ? std::vector<Seg>{} : cmap, j ? 0 : cin_phys);
    for (int blk = 2; blk <= 5; ++blk) {
      for (int j = 0; j < 3; ++j)
        b.conv("Mconv" + std::to_string(blk) + "_" + tag + "_" + std::to_string(j), j ? oth : cur,
               j ? (j - 1) * w : 0, oth, j * w);
      std::swap(cur, oth);
    }
    b.conv("Mconv6_" + tag, cur, 0, T6, 0);
    b.conv("Mconv7_" + tag, T6, 0, out, out_coff);
  };
  // model.py:183-190: L2 stages; stage 0 sees out0, stages 1-3 cat(out0, paf)
  stage("stage0_L2", 96, {{0, 0, 128}}, 128, SIN, 128);
  for (int s = 1; s < 4; ++s) stage("stage" + std::to_string(s) + "_L2", 128, {{0, 0, 180}}, 184, SIN, 128);
  // model.py:193-198: L1 stage 0 on cat(out0, paf)
  stage("stage0_L1", 96, {{0, 0, 180}}, 184, SIN, 184);
  // model.py:199-205: L1 stage 1 on cat(out0, heat0, paf) — logical order mapped onto physical slices
  stage("stage1_L1", 128, {{0, 0, 128}, {128, 184, 26}, {154, 128, 52}}, 216, HOUT, 0);
  net->out0 = {SIN, 128, 52};
  net->out1 = {HOUT, 0, 26};
  net->n_out = 2;
}

static void build_coco(isl_net* net) {
  Builder b{net};
  const int X = b.buf(0, 8, 1);
  net->in_buf = X;
  // stage input: [L1 0:38 (gap 40) | L2 40:59 (gap 64) | out1 64:192]; 7x7 consumers -> ring 3
  const int SIN = b.buf(3, 192, 3), T1 = b.buf(3, 128, 3), T2 = b.buf(3, 128, 3);
  const int T5a = b.buf(3, 512, 1), T5b = b.buf(3, 512, 1), T6a = b.buf(3, 128, 1), T6b = b.buf(3, 128, 1);
  b.front(X, false, SIN, 64, 3);
  // stage 1 (model.py:306-308): both branches read out1, write their slices last
  for (int br = 1; br <= 2; ++br) {
    const std::string s = "_L" + std::to_string(br);
    b.conv("conv5_1_CPM" + s, SIN, 64, T1, 0);
    b.conv("conv5_2_CPM" + s, T1, 0, T2, 0);
    b.conv("conv5_3_CPM" + s, T2, 0, T1, 0);
    b.conv("conv5_4_CPM" + s, T1, 0, br == 1 ? T5a : T5b, 0);
  }
  b.conv("conv5_5_CPM_L1", T5a, 0, SIN, 0);
  b.conv("conv5_5_CPM_L2", T5b, 0, SIN, 40);
  const std::vector<Seg> cmap = {{0, 0, 38}, {38, 40, 19}, {57, 64, 128}};  // cat(L1, L2, out1)
  for (int i = 2; i <= 6; ++i) {
    for (int br = 1; br <= 2; ++br) {
      const std::string s = "_stage" + std::to_string(i) + "_L" + std::to_string(br);
      b.conv("Mconv1" + s, SIN, 0, T1, 0, cmap, 192);
      b.conv("Mconv2" + s, T1, 0, T2, 0);
      b.conv("Mconv3" + s, T2, 0, T1, 0);
      b.conv("Mconv4" + s, T1, 0, T2, 0);
      b.conv("Mconv5" + s, T2, 0, T1, 0);
      b.conv("Mconv6" + s, T1, 0, br == 1 ? T6a : T6b, 0);
    }
    // both branches have consumed SIN; now overwrite its L1/L2 slices
    b.conv("Mconv7_stage" + std::to_string(i) + "_L1", T6a, 0, SIN, 0);
    b.conv("Mconv7_stage" + std::to_string(i) + "_L2", T6b, 0, SIN, 40);
  }
  net->out0 = {SIN, 0, 38};
  net->out1 = {SIN, 40, 19};
  net->n_out = 2;
}

static void build_hand(isl_net* net) {
  Builder b{net};
  const int X = b.buf(0, 8, 1);
  net->in_buf = X;
  // stage input: [stage output 0:22 (gap 24) | out1_0 24:152]
  const int SIN = b.buf(3, 152, 3), T1 = b.buf(3, 128, 3), T2 = b.buf(3, 128, 3);
  const int T5 = b.buf(3, 512, 1), T6 = b.buf(3, 128, 1);
  b.front(X, true, SIN, 24, 3);
  b.conv("conv6_1_CPM", SIN, 24, T5, 0);
  b.conv("conv6_2_CPM", T5, 0, SIN, 0);
  const std::vector<Seg> cmap = {{0, 0, 22}, {22, 24, 128}};  // cat(prev, out1_0), model.py:397-405
  for (int i = 2; i <= 6; ++i) {
    const std::string s = "_stage" + std::to_string(i);
    b.conv("Mconv1" + s, SIN, 0, T1, 0, cmap, 152);
    b.conv("Mconv2" + s, T1, 0, T2, 0);
    b.conv("Mconv3" + s, T2, 0, T1, 0);
    b.conv("Mconv4" + s, T1, 0, T2, 0);
    b.conv("Mconv5" + s, T2, 0, T1, 0);
    b.conv("Mconv6" + s, T1, 0, T6, 0);
    b.conv("Mconv7" + s, T6, 0, SIN, 0);
  }
  net->out0 = {SIN, 0, 22};
  net->n_out = 1;
}

// Fusable 1x1 pairs (conv_x3 VAR 16): op k and op k + 1 both 1x1 convs, op k + 1 reading the
// whole output of op k (offset 0, identity channel map) from a buffer no other op reads before
// it is written again and that is no net output, shapes with a fused variant (x3_fused67_fits).  body_25's six
// Mconv6 -> Mconv7 pairs and the hand's conv6_1/6_2 and Mconv6/7 pairs; COCO's pairs are not
// adjacent (both branches read the stage input before either Mconv7 overwrites it).
static void plan_fuse67(isl_net* net) {
  for (size_t k = 0; k + 1 < net->ops.size(); ++k) {
    Op& a = net->ops[k];
    const Op& b = net->ops[k + 1];
    if (a.type != 0 || b.type != 0) continue;
    ConvLayer& la = net->layers[a.layer];
    ConvLayer& lb = net->layers[b.layer];
    if (la.k != 1 || lb.k != 1 || b.in != a.out || b.in_coff != 0 || a.out_coff != 0) continue;
    if (lb.cin != la.cout || lb.cin_phys != la.cout || lb.cmap.size() != 1 || lb.cmap[0].logical != 0 ||
        lb.cmap[0].phys != 0 || !x3_fused67_fits(la.cout, lb.cout))
      continue;
    if (net->out0.buf == a.out || (net->n_out > 1 && net->out1.buf == a.out)) continue;
    // the value op k writes is read by op k + 1 only: no later op reads the buffer before the
    // next op that writes it (every stage's Mconv6 reuses one buffer)
    // channel by channel: a later op may read the buffer only where a later write has replaced
    // op k's value (the fused launch never writes Mconv6's channels)
    bool other = false;
    std::vector<char> live(la.cout, 1);
    int n_live = la.cout;
    for (size_t j = k + 2; j < net->ops.size() && n_live > 0 && !other; ++j) {
      const Op& o = net->ops[j];
      if (o.in == a.out) {
        const int rc = o.type == 0 ? net->layers[o.layer].cin_phys : o.C;
        for (int ch = std::max(0, o.in_coff); ch < std::min(la.cout, o.in_coff + rc); ++ch) other |= live[ch] != 0;
      }
      if (o.out == a.out) {
        const int wc = o.type == 0 ? net->layers[o.layer].cout : o.C;
        for (int ch = std::max(0, o.out_coff); ch < std::min(la.cout, o.out_coff + wc); ++ch)
          if (live[ch]) { live[ch] = 0; --n_live; }
      }
    }
    if (other) continue;
    a.fuse67 = true;
    la.fuse6 = true;
    lb.fuse7 = true;
  }
}

// ISLPOSE_X3_FUSE67: 0 the pairs as two plain launches (natural channel order; A/B), 2 always
// fused, 3 always the permuted two launches (tests), default by grid (x3_fused67_grid).  ISL_PREC_FP16 (h16): the one-term forms of both exist, but the fused K order of Mconv7
// is the permuted one, not the natural order of the mode's plain launches (round-off apart), so
// there an unset switch keeps the plain launches (0); 1 selects by grid as the fp32 default does
static int fuse67_mode(const X3Switches& sw, bool h16) { return sw.fuse67 >= 0 ? sw.fuse67 : h16 ? 0 : 1; }

// What the run does with the fusable pair (op k, op k + 1) under mode f67: 0 the plain launches,
// 1 the fused launch, 2 the permuted two launches -- only where Mconv7 has K ranges (canonical:
// its ranges are the fused kernel's wave shares, so both forms give the same bits); larger planes
// always fuse.  `act`: the plan's geometry.
static ConvLaunch basic_launch(const isl_net* net, const std::vector<Act>& act, const Op& op);
static int fuse67_form(const isl_net* net, const std::vector<Act>& act, size_t k, int f67, int cus, const X3Switches& sw) {
  const Op& op = net->ops[k];
  if (!f67 || !op.fuse67) return 0;
  if ((f67 == 3 || (f67 == 1 && !x3_fused67_grid(basic_launch(net, act, op), cus))) &&
      x3_split_ranges(basic_launch(net, act, net->ops[k + 1]), nullptr, cus, sw) > 1)
    return 2;
  return 1;
}

static void drop_all_graphs(isl_net* net);

// Every weight buffer goes up through here: allocated on first use, the same size ever after
// (a layer's shape is fixed), copied by a blocking copy
static int upload(DevBuf& d, const void* host, size_t bytes) {
  if (!d.p) {
    HIP_OK(hipMalloc(&d.p, bytes));
    d.bytes = bytes;
  }
  if (d.bytes != bytes) return fail(ISL_E_STATE, "weight upload: buffer size changed");
  HIP_OK(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice));
  return ISL_OK;
}

// Build and upload the packs every layer owns (owns_pack), full or hi-only.  A layer has one
// 2^s, PK_X3's: the packs the kernels read beside it must reproduce it.
static int upload_packs(isl_net* net, bool hi) {
  for (ConvLayer& c : net->layers)
    for (int kind = 0; kind < PK_COUNT; ++kind) {
      if (!owns_pack(c, kind) || (hi && !pack_has_hi(kind))) continue;
      float inv = 1.f;
      const HostPack hp = build_pack(c, kind, hi, &inv);
      const char* same = kind == PK_X3F7 ? "Mconv7 scale mismatch" : kind == PK_X3P ? "permuted scale mismatch"
                         : kind == PK_X3 && hi ? "scale mismatch" : nullptr;
      if (same && inv != c.inv[PK_X3]) return fail(ISL_E_STATE, std::string(hi ? "hi-only pack: " : "fused pair: ") + same);
      if (!hi) c.inv[kind] = inv;
      if (const int rc = upload(c.dev[kind][hi], hp.data(), hp.bytes())) return rc;
    }
  return ISL_OK;
}

// ISL_PREC_FP16's filters: built when a run first needs them after a weight upload (at the
// upload itself when the mode is already selected), kept across precision switches
static int upload_hi_packs(isl_net* net) {
  if (const int rc = upload_packs(net, true)) return rc;
  net->packed_hi = true;
  return ISL_OK;
}

static int upload_params(isl_net* net) {
  drop_all_graphs(net);   // new weight scales: the captured launches' arguments are stale
  net->packed_hi = false; // both packs follow the weights
  for (ConvLayer& c : net->layers) {
    if (!c.has_w || !c.has_b || (c.act == ACT_PRELU && !c.has_s))
      return fail(ISL_E_STATE, "parameter missing for layer " + c.name);
    for (int p = 0; p < PB_COUNT; ++p) {
      if (p >= PB_BIAS_PERM && !c.fuse6) continue;   // Mconv6 of a pair's permuted two-launch form
      const std::vector<float> v = build_param(c, p, param_pad(c));
      if (const int rc = upload(c.par[p], v.data(), v.size() * sizeof(float))) return rc;
    }
  }
  if (const int rc = upload_packs(net, false)) return rc;
  // the flags are zeroed by blocking copies (complete on return, like the weight uploads above),
  // so every later run on any stream sees them zeroed -- no device-wide drain
  if (!net->d_flag) {
    const int zero = 0;
    HIP_OK(hipMalloc(&net->d_flag, sizeof(int)));
    HIP_OK(hipMemcpy(net->d_flag, &zero, sizeof(int), hipMemcpyHostToDevice));
  }
  if (!net->d_trips) {
    const unsigned long long zero = 0;
    HIP_OK(hipMalloc(&net->d_trips, sizeof(unsigned long long)));
    HIP_OK(hipMemcpy(net->d_trips, &zero, sizeof(zero), hipMemcpyHostToDevice));
  }
  net->packed = true;
  return ISL_OK;
}

// Activation arenas: one per net input size (h, w), sized by frame capacity, so
// the scales of a pyramid (or the 4 hand scales) keep their own arena instead of
// reallocating per call, and a batch of n frames reuses an arena that holds
// n' >= n (the buffers of the n'-frame layout hold any n <= n' frames; their
// rings and gap channels were zeroed once and no kernel writes them).  A larger n
// replaces the arena of its size; arenas of other sizes are evicted least-recently-
// used when the net's total would pass the budget.  Variable crop counts
// (HandEstimator.estimate_crops) therefore cost at most one arena per hand scale,
// of the largest count seen.
static size_t arena_budget() {
  static const size_t b = [] {
    const char* e = getenv("ISLPOSE_ARENA_BUDGET_MB");
    const long long mb = e ? atoll(e) : 65536;
    return (size_t)(mb > 0 ? mb : 65536) << 20;
  }();
  return b;
}

// Instantiated graphs hold the pointers and scalars of the launches they captured: any
// reallocation of a buffer they name (arena, split-K workspace, weights re-uploaded with new
// scales) drops them.  A replay may still be queued on any stream (the caller's, not ours), so
// a drop drains the device before the execs are destroyed: drops are rare (weights, workspace
// growth, arena eviction), the wait is cheap next to them.
// The per-arena cap's evictions (run_ops) do not drain the device on the launch path: the
// evicted exec is retired behind the event recorded after its latest replay and destroyed once
// that event has passed (reap_graphs, at the next run_ops); a retired exec is never launched again.
static void free_graph(isl_net::Arena::Graph& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.done) (void)hipEventDestroy(g.done);
  g.exec = nullptr;
  g.done = nullptr;
}

static int reap_graphs(isl_net::Arena& ar) {
  auto& v = ar.graph_retired;
  for (size_t i = 0; i < v.size();) {
    const hipError_t q = v[i].done ? hipEventQuery(v[i].done) : hipSuccess;
    if (q == hipSuccess) {
      free_graph(v[i]);
      v[i] = v.back();
      v.pop_back();
    } else if (q == hipErrorNotReady) {
      // a not-ready query leaves hipErrorNotReady behind: clear that one only (an unrelated
      // sticky error of the caller's stays for them to see)
      (void)hipGetLastError();
      ++i;
    } else {
      return fail(ISL_E_HIP, std::string("graph retirement: ") + hipGetErrorString(q));
    }
  }
  return ISL_OK;
}

// A drop waits for the latest replay of every exec (its `done` event, recorded behind the replay
// on the caller's stream) instead of draining the device; the failed-capture set is cleared too,
// so a transient capture failure does not keep a key eager past a weight reload or a workspace
// change.
static void drop_graphs(isl_net::Arena& ar) {
  for (auto& kv : ar.graphs)
    if (kv.second.done) (void)hipEventSynchronize(kv.second.done);
  for (auto& g : ar.graph_retired)
    if (g.done) (void)hipEventSynchronize(g.done);
  for (auto& kv : ar.graphs) free_graph(kv.second);
  for (auto& g : ar.graph_retired) free_graph(g);
  ar.graphs.clear();
  ar.graph_retired.clear();
  ar.graph_failed.clear();
}

static void drop_all_graphs(isl_net* net) {
  for (auto& kv : net->plans) drop_graphs(kv.second);
}

static void drop_arena(isl_net* net, std::map<long long, isl_net::Arena>::iterator it) {
  drop_graphs(it->second);
  // hipFree waits for queued work that may still use the arena
  (void)hipFree(it->second.base);
  if (it->second.tab) (void)hipFree(it->second.tab);
  if (it->second.tab_ev) {
    (void)hipEventSynchronize(it->second.tab_ev);
    (void)hipEventDestroy(it->second.tab_ev);
  }
  if (it->second.tab_pin) (void)hipHostFree(it->second.tab_pin);
  if (it->second.ks) (void)hipFree(it->second.ks);
  if (it->second.fold_mem) (void)hipFree(it->second.fold_mem);
  if (it->second.fold_tab) (void)hipFree(it->second.fold_tab);
  net->plans_bytes -= it->second.bytes;
  if (net->arena == it->second.base) {
    net->arena = nullptr;
    net->cur = nullptr;
    net->pn = net->ph = net->pw = 0;
  }
  net->plans.erase(it);
}

// The buffers of an n-frame plan at net size h x w (no addresses yet).  a16: an fp16-storage arena
// (ISL_ACT_FP16) -- every buffer between the convs holds fp16 (Act::esize 2), the net input and the
// net outputs' own buffers stay fp32; those output buffers take no bytes in an fp32 arena.
static std::vector<Act> layout_acts(const isl_net* net, int n, int h, int w, bool a16) {
  const int lh[4] = {h, h / 2, h / 4, h / 8}, lw[4] = {w, w / 2, w / 4, w / 8};
  std::vector<Act> act(net->bufs.size());
  for (size_t i = 0; i < net->bufs.size(); ++i) {
    const BufSpec& b = net->bufs[i];
    Act& a = act[i];
    a.n = b.out32 && !a16 ? 0 : n;
    a.H = lh[b.level]; a.W = b.half ? lw[b.level] / 2 : lw[b.level]; a.pad = b.pad; a.cs = b.cs;
    a.esize = a16 && !b.out32 && (int)i != net->in_buf ? 2 : 4;
  }
  return act;
}

static bool act16_plan_ok(const isl_net* net, const std::vector<Act>& geo);

// Whether an n-frame run at h x w stores its activations as fp16: the switch is on, it applies
// (ISL_ALGO_X3 with ISL_PREC_FP16) and every step of the run's launch plan on the fp16 geometry
// has an fp16-storage form -- all or nothing, decided before the first launch (act16_plan_ok).
static bool act16_for(const isl_net* net, int n, int h, int w) {
  if (net->act_storage != ISL_ACT_FP16 || net->algo != ISL_ALGO_X3 || net->precision != ISL_PREC_FP16) return false;
  return act16_plan_ok(net, layout_acts(net, n, h, w, true));
}

static int plan(isl_net* net, int n, int h, int w, hipStream_t s) {
  if (n <= 0 || h < 8 || w < 8) return fail(ISL_E_ARG, "net input must be at least 8x8 with n >= 1");
  // arenas by (net size, storage)
  const bool a16 = act16_for(net, n, h, w);
  const long long key = ((long long)h << 20) | w | (a16 ? 1LL << 62 : 0);
  auto it = net->plans.find(key);
  if (it != net->plans.end() && it->second.n_cap < n) {
    drop_arena(net, it);
    it = net->plans.end();
  }
  if (it == net->plans.end()) {
    isl_net::Arena ar;
    ar.n_cap = n;
    ar.a16 = a16;
    for (const Act& a : layout_acts(net, n, h, w, a16)) {
      ar.offs.push_back(ar.bytes);
      ar.bytes += (a.bytes() + 255) / 256 * 256;
    }
    // LRU eviction of the other sizes' arenas over the budget
    while (net->plans_bytes + ar.bytes > arena_budget() && !net->plans.empty()) {
      auto lru = net->plans.begin();
      for (auto j = net->plans.begin(); j != net->plans.end(); ++j)
        if (j->second.last_use < lru->second.last_use) lru = j;
      drop_arena(net, lru);
    }
    HIP_OK(hipMalloc(&ar.base, ar.bytes));
    // zero rings and gap channels, once, on the caller's stream: the work that follows on that
    // stream (this call's preprocess / pack and run) is ordered behind it.  (Round 5 zeroed on
    // the null stream, which torch's non-blocking streams do not wait for, and then drained the
    // whole device; the ordering is what the first-run race needed, VERDICT r05 #4.)
    HIP_OK(hipMemsetAsync(ar.base, 0, ar.bytes, s));
    net->plans_bytes += ar.bytes;
    it = net->plans.emplace(key, std::move(ar)).first;
  }
  isl_net::Arena& ar = it->second;
  ar.last_use = ++net->plan_clock;
  net->cur = &ar;
  net->a16_active = ar.a16;
  if (net->arena == ar.base && net->pn == n && net->ph == h && net->pw == w) return ISL_OK;
  net->act = layout_acts(net, n, h, w, ar.a16);
  for (size_t i = 0; i < net->bufs.size(); ++i) net->act[i].base = (float*)((char*)ar.base + ar.offs[i]);
  net->arena = ar.base;
  net->pn = n; net->ph = h; net->pw = w;
  return ISL_OK;
}

// Conv algorithm of a net (isl_net_set_algo); ISLPOSE_CONV_ALGO=x3|wino|direct
// sets the default at isl_net_create (A/B tests).
static int default_algo() {
  const char* e = getenv("ISLPOSE_CONV_ALGO");
  if (!e) return ISL_ALGO_X3;
  if (e[0] == 'w') return ISL_ALGO_WINO;
  if (e[0] == 'd') return ISL_ALGO_DIRECT;
  return ISL_ALGO_X3;
}

// Precision of a net's ISL_ALGO_X3 convs (isl_net_set_precision); ISLPOSE_PRECISION=fp32|fp16
// sets the default at isl_net_create (unset or anything else: fp32).
static int default_precision() {
  const char* e = getenv("ISLPOSE_PRECISION");
  return e && std::string(e) == "fp16" ? ISL_PREC_FP16 : ISL_PREC_FP32;
}

// Activation storage of a net's ISL_PREC_FP16 convs (isl_net_set_act_storage);
// ISLPOSE_ACT_STORAGE=fp32|fp16 sets the default at isl_net_create (unset or anything else: fp32).
static int default_act_storage() {
  const char* e = getenv("ISLPOSE_ACT_STORAGE");
  return e && std::string(e) == "fp16" ? ISL_ACT_FP16 : ISL_ACT_FP32;
}

#ifdef ISLPOSE_DEV
// ISL_ALGO_X3 runs 3x3 layers on the direct split-fp16 kernel; ISLPOSE_X3_WINO=1
// selects the split-fp16 Winograd kernel instead.  It is fp32-accurate (rel err
// 3e-6) but measured 1.3-1.8x SLOWER (r01): its V transform + split costs ~184
// VALU ops per (tile, channel), twice the time of the 6144 MFMA FLOPs they feed
// at 64 output channels per block, and a 128 KB single-buffered step leaves
// no room for more channels.  Kept for A/B and as the record of that finding.
static bool x3_wino_enabled(const X3Switches& sw) { return sw.x3_wino != 0; }
#endif

// 3x3 layers on chip-filling grids through the split-fp16 Winograd F(2x2, 3x3) kernel
// (wino_f16.hip: 2.25x fewer MFMAs, fp32-accurate like conv_x3) where wino_f16_fits;
// ISLPOSE_X3_W2=0: conv_x3 everywhere (A/B)
// Default: layers with >= 256 input channels (32 chunks) -- measured faster than conv_x3 there
// (46x82 c384->128 1.06-1.16x, 92x164 c256->256 1.04-1.12x, 46x82 c512->512 1.05-1.17x in
// tools/convbench, profiles/r06/w2c/), slower on c128->128 (K = 128: 0.85-0.9x).
// ISLPOSE_X3_W2=0 never, =1 every eligible launch (A/B, tests), default 2 = the K rule.
static int w2_mode(const X3Switches& sw) { return sw.w2; }
static bool w2_enabled(const X3Switches& sw, const ConvLaunch& c) {
  const int m = w2_mode(sw);
  return m == 1 || (m == 2 && c.cin_chunks >= 32);
}

// The plan-level switches (x3_switches(), read once per run by plan_steps, so a test can compare
// both settings in one process):
// ISLPOSE_RGB_CONV=0: conv1_1 on the generic split-fp16 kernel (A/B)
static bool rgb_kernel_enabled(const X3Switches& sw) { return sw.rgb_conv != 0; }
// conv1_1 -> conv1_2 -> the 2x2 pool in one launch (conv_c12.hip) writing the pooled map;
// ISLPOSE_C12=0: the two convs as their own launches, =2: the fused launch writing the pool's
// pair-max buffer, finished by the next conv's staging (round-5 form; A/B)
static int c12_mode(const X3Switches& sw) { return sw.c12; }
// ISLPOSE_FUSED_POOL=0: the plain conv + maxpool2 path (A/B)
static bool fused_pool_enabled(const X3Switches& sw) { return sw.fused_pool != 0; }
// ISLPOSE_POOL_INPUT=0: a fused pool's row-pair max runs as vpool2_kernel into the pooled
// buffer instead of inside the next conv's staging (ConvLaunch::vin; A/B)
static bool pool_input_enabled(const X3Switches& sw) { return sw.pool_input != 0; }

// Pool op k may leave its output unwritten and hand its pair-max buffer to op k+1 (vin):
// op k+1 is an x3 conv (not the 3-channel rgb kernel) reading the whole pooled buffer,
// which nothing else reads and which is no net output.
static bool pool_into_next_conv(const isl_net* net, const std::vector<Act>& act, size_t k) {
  const Op& op = net->ops[k];
  if (k + 1 >= net->ops.size() || net->algo != ISL_ALGO_X3) return false;
  const Op& nx = net->ops[k + 1];
  if (nx.type != 0 || nx.in != op.out || nx.in_coff != 0) return false;
  const ConvLayer& c = net->layers[nx.layer];
  if (c.cin_phys / 8 == 1 || act[op.out].pad < c.k / 2 || act[op.out].cs != (op.C + 7) / 8 * 8)
    return false;
  if (net->out0.buf == op.out || (net->n_out > 1 && net->out1.buf == op.out)) return false;
  // the staging addresses the pair-max buffer as [chunk][2H][W][8] of the pooled H x W: a
  // pre-pool plane of odd height (floor-mode pool drops its last row) has another chunk
  // stride, so it takes vpool2 (e.g. 8 x 372 x 656, level-2 height 93)
  if (act[op.in].H != 2 * act[op.out].H || act[op.in].W != 2 * act[op.out].W) return false;
  for (size_t j = 0; j < net->ops.size(); ++j)
    if (j != k + 1 && (net->ops[j].in == op.out || (j != k && net->ops[j].out == op.out))) return false;
  return true;
}

// ISLPOSE_X3_FOLD=1: split-K producers leave their partials to folding consumers (A/B).  Off by default: at batch 1 (Mode R) the consumers' staging re-reads S partials
// per element and kernel row, and the frame ran 427 -> 315 frames/s (profiles/r03/fold_ab/)
static bool fold_enabled() {
#ifdef ISLPOSE_DEV
  return x3_switches().fold != 0;
#else
  return false;   // rejected: development build only
#endif
}

// The conv launch of an op on the geometry `act` before the per-run adjustments (pools, wide 1x1
// tiles, fold)
static ConvLaunch basic_launch(const isl_net* net, const std::vector<Act>& act, const Op& op) {
  const Act& in = act[op.in];
  const Act& out = act[op.out];
  const ConvLayer& c = net->layers[op.layer];
  ConvLaunch L;
  L.in = in.base; L.in_pad = in.pad; L.in_cs = in.cs; L.in_coff = op.in_coff;
  L.out = out.base; L.out_pad = out.pad; L.out_cs = out.cs; L.out_coff = op.out_coff;
  L.wpk = (const float*)c.pack(PK_DIRECT); L.bias = c.param(PB_BIAS); L.slope = c.param(PB_SLOPE);
  L.n = in.n; L.H = in.H; L.W = in.W; L.ks = c.k; L.cin_chunks = c.cin_phys / 8;
  L.cout = c.cout; L.bco = c.bco; L.act = c.act;
  L.wx3 = c.pack(PK_X3); L.wscale_inv = c.inv[PK_X3]; L.range_flag = net->d_flag;
  L.allow_split = net->split_k;
  return L;
}

// Whether ops k, k + 1, k + 2 (conv1_1 on the rgb kernel, conv1_2, the pool) run as the one
// conv_c12.hip launch: conv1_1's output feeds conv1_2 only.  0: no; 1: the launch writes the pool's
// pair-max buffer (ISLPOSE_C12=2, or no pooled buffer of the floor-mode shape); 2: the whole pool in
// the epilogue.  *l1 / *l2 are the launches (h16: the one-term form from the hi-only packs, a16:
// its fp16 output) on the geometry `act`.
static int c12_form(const isl_net* net, const std::vector<Act>& act, size_t k, bool fuse_pools, bool h16, bool a16,
                    int cus, const X3Switches& sw, ConvLaunch* l1, ConvLaunch* l2) {
  const Op& op = net->ops[k];
  const int c12m = c12_mode(sw);
  if (!(net->algo == ISL_ALGO_X3 && op.type == 0 && fuse_pools && c12m && k + 2 < net->ops.size() &&
        rgb_layer(net->layers[op.layer]) && rgb_kernel_enabled(sw)))
    return 0;
  const Op& o2 = net->ops[k + 1];
  const Op& pl = net->ops[k + 2];
  bool only = o2.type == 0 && o2.in == op.out && o2.in_coff == 0 && op.out_coff == 0 && pl.type == 1 &&
              pl.in == o2.out && o2.out_coff == 0 && pl.hbuf >= 0 && net->out0.buf != op.out &&
              !(net->n_out > 1 && net->out1.buf == op.out);
  for (size_t j = k + 2; only && j < net->ops.size(); ++j) {
    if (net->ops[j].in == op.out) only = false;
    if (net->ops[j].out == op.out) break;
  }
  if (!only) return 0;
  ConvLaunch L1 = basic_launch(net, act, op), L2 = basic_launch(net, act, o2);
  L1.wx3 = net->layers[op.layer].pack(PK_RGB, h16);
  if (h16) {   // the one-term form: the hi-only packs of both layers
    L2.wx3 = net->layers[o2.layer].pack(PK_X3, true);
    L1.f16 = L2.f16 = 1;
    L1.act16 = L2.act16 = a16 ? 1 : 0;   // (the pooled map / pair-max buffer is fp16)
  }
  const Act& hb = act[pl.hbuf];
  L2.out = hb.base; L2.out_pad = 0; L2.out_cs = hb.cs; L2.out_coff = 0;
  L2.hpool = 1;
  if (!(pl.C == L2.cout && x3_rgb_fits(L1) && x3_hpool_ok(L2, cus, sw) && x3_c12_fits(L1, L2))) return 0;
  // the whole pool in the epilogue: the pooled buffer is the floor-mode 2x2 pool of conv1_2's
  // plane, written from its channel 0
  const Act& po = act[pl.out];
  int form = 1;
  if (c12m == 1 && pl.out_coff == 0 && po.H == L2.H / 2 && po.W == L2.W / 2 && po.cs >= 64 && po.n == L2.n) {
    ConvLaunch P = L2;
    P.out = po.base; P.out_pad = po.pad; P.out_cs = po.cs; P.hpool = 2;
    if (x3_c12_fits(L1, P)) { L2 = P; form = 2; }
  }
  *l1 = L1; *l2 = L2;
  return form;
}

// One step of a run's launch plan (plan_steps): a pool, a conv launch, or a launch that swallows
// the ops after it (the fused 1x1 pair: 2 ops; conv1_1 -> conv1_2 [-> pool]: 2 or 3).
struct Step {
  enum Kind {
    POOL, VPOOL,     // maxpool2 / the row-pair half of a pool whose conv wrote the pair-max buffer
    POOL_DEFERRED,   // no launch: the next conv stages from the pair-max buffer (ConvLaunch::vin)
    X3, X3_RGB, W2, PAIR, C12,
    DIRECT, WINO,    // from here on: convs off the x3 kernels -- the fp32 kernels
#ifdef ISLPOSE_DEV
    WINO_X3,
#endif
  };
  Kind kind = POOL;
  int op = 0, nops = 1;      // the first op and how many the step covers
  ConvLaunch L{}, L2{};      // the launch (C12: conv1_1 and conv1_2), but for the split-K workspace and fold pointers
  X3Choice choice{};         // X3, X3_RGB, PAIR: what the launch runs (x3_choose)
  int code[3] = {0, 0, 0};   // op_variant of the covered ops (the first of X3, X3_RGB, PAIR: the choice's code)
  int late_pool = -1;        // a deferred pool this conv has no pooled-input variant for: its vpool2 runs first
  bool covered = false;      // the step has an fp16-storage form (ISL_ACT_FP16)
  const char* error = nullptr;   // ISL_E_STATE: the run cannot take this step
};

// The launch plan of a run on the geometry `act`: what every op becomes, in order, with its
// launch filled in.  A pure host function of its arguments, the device's CU count and the
// ISLPOSE_* switches, which it reads once (x3_switches) and returns in *sw_out -- the run
// (run_ops_eager, on net->act) and the storage decision (act16_plan_ok, on a trial geometry
// without addresses) both read it.  h16: ISL_PREC_FP16 (ISL_ALGO_X3 only), every x3 conv on the
// one-term form of the variant the fp32 plan picks, from the hi-only packs -- the conv1_1 ->
// conv1_2 launch included (the same bits as its layers); the fused 1x1 pair only where
// ISLPOSE_X3_FUSE67 asks for it (fuse67_mode); the Winograd kernel is never chosen.  a16: `act`
// holds fp16 between the convs, the launches are those of the fp32-storage run on the
// fp16-storage forms.  far: the arena whose fold plan (plan_fold) applies, or null.
static std::vector<Step> plan_steps(const isl_net* net, const std::vector<Act>& act, bool h16, bool a16,
                                    const isl_net::Arena* far, X3Switches* sw_out = nullptr) {
  const X3Switches sw = x3_switches();
  if (sw_out) *sw_out = sw;
  const int cus = device_cus();
  const size_t nops = net->ops.size();
  std::vector<Step> steps;
  steps.reserve(nops);
  bool fused = false;   // the previous conv wrote the pair-max buffer of this pool
  int vin_buf = -1;     // this conv stages from that buffer (the pool op was skipped)
  const bool fuse_pools = fused_pool_enabled(sw), pool_input = fuse_pools && pool_input_enabled(sw);
  const int f67 = net->algo == ISL_ALGO_X3 ? fuse67_mode(sw, h16) : 0;
  size_t perm_op = (size_t)-1;   // the pair (perm_op, perm_op + 1) runs as its permuted two launches
  // fp16 storage: the layer that writes a net output last also keeps the unrounded fp32 values
  auto store16 = [&](ConvLaunch& L, size_t writer) {
    L.act16 = 1;
    for (int o = 0; o < net->n_out; ++o)
      if ((int)writer == net->out_op[o]) {
        const Act& ob = act[net->out32_buf[o]];
        L.out32 = ob.base; L.out32_pad = ob.pad; L.out32_cs = ob.cs;
      }
  };
  for (size_t k = 0; k < nops; k += steps.back().nops) {
    const Op& op = net->ops[k];
    steps.emplace_back();
    Step& st = steps.back();
    ConvLaunch& L = st.L;
    st.op = (int)k;
    const int form67 = vin_buf < 0 ? fuse67_form(net, act, k, f67, cus, sw) : 0;
    if (form67 == 2) perm_op = k;
    if (form67 == 1) {
      // Mconv6 -> Mconv7 in one launch (conv_x3 VAR 16): op k's input, op k + 1's output
      const Op& op7 = net->ops[k + 1];
      const ConvLayer& c6 = net->layers[op.layer];
      const ConvLayer& c7 = net->layers[op7.layer];
      const Act& o7 = act[op7.out];
      L = basic_launch(net, act, op);
      L.out = o7.base; L.out_pad = o7.pad; L.out_cs = o7.cs; L.out_coff = op7.out_coff;
      L.wx3 = c6.pack(c6.pair6_kind(), h16);
      L.wx3f7 = c7.pack(PK_X3F7, h16); L.bias7 = c7.param(PB_BIAS); L.slope7 = c7.param(PB_SLOPE);
      L.wscale7_inv = c7.inv[PK_X3];
      L.cout7 = c7.cout; L.act7 = c7.act;
      if (h16) L.f16 = 1;
      if (a16) store16(L, k + 1);
      st.kind = Step::PAIR;
      st.nops = 2;
      st.code[1] = -2;   // ran inside op k
      // (the net input is fp32 in every arena: only the 3-channel kernel reads it)
      st.choice = x3_choose(L, cus, sw);
      st.code[0] = st.choice.code;
      st.covered = op.in != net->in_buf && st.choice.act16;
      continue;
    }

    // conv1_1 (rgb kernel) -> conv1_2 -> pool: both convs and the pool in one launch writing the
    // pooled map (or, ISLPOSE_C12=2, the pool's pair-max buffer), where conv1_1's output feeds
    // conv1_2 only (conv_c12.hip; its fp16-storage form reads the fp32 net input)
    const int form12 = vin_buf < 0 ? c12_form(net, act, k, fuse_pools, h16, a16, cus, sw, &st.L, &st.L2) : 0;
    if (form12) {
      st.kind = Step::C12;
      st.nops = form12 == 2 ? 3 : 2;   // 2: the pool ran inside op k too; 1: the pool op finds its pair-max buffer written
      if (form12 == 1) fused = true;
      // (ISL_PREC_FP16 also sets X3V_RGB: conv1_1 runs conv_x3_rgb's one-term K packing inside the
      // launch, and the fp16 suites find the 3-channel form of a run by that bit)
      st.code[0] = x3_variant_code(X3V_C12 | (h16 ? X3V_F16 | X3V_RGB : 0) | (a16 ? X3V_A16 : 0), 3, 256, 64);
      // conv1_2 ran inside op k.  ISL_PREC_FP16 reports it as -1, "fused with its pool": the
      // fp16-storage suite holds every conv op of a run to the act16 bit or that code
      st.code[1] = h16 ? -1 : -2;
      st.code[2] = -2;
      st.covered = true;
      continue;
    }

    if (op.type == 1) {
      // deferred: the next conv either stages from the pair-max buffer or runs vpool2 first
      if (fused && pool_input && pool_into_next_conv(net, act, k)) {
        vin_buf = (int)k;
        st.kind = Step::POOL_DEFERRED;
        st.code[0] = -1;
      } else {
        st.kind = fused ? Step::VPOOL : Step::POOL;
      }
      fused = false;
      st.covered = true;
      continue;
    }
    const ConvLayer& c = net->layers[op.layer];
    L = basic_launch(net, act, op);
    if (net->algo == ISL_ALGO_WINO && c.wbco) {
      L.wpk = (const float*)c.pack(PK_WINO); L.bco = c.wbco;
      st.kind = Step::WINO;
#ifdef ISLPOSE_DEV
    } else if (net->algo == ISL_ALGO_X3 && owns_pack(c, PK_WINO_X3) && x3_wino_enabled(sw) && vin_buf < 0) {
      L.wx3 = c.pack(PK_WINO_X3); L.wscale_inv = c.inv[PK_WINO_X3];
      st.kind = Step::WINO_X3;
#endif
    } else if (net->algo == ISL_ALGO_X3 && x3_fits(L)) {
      if (vin_buf >= 0) {   // the preceding pool's row-pair max happens in this conv's staging
        const Act& hb = act[net->ops[vin_buf].hbuf];
        ConvLaunch Lv = L;
        Lv.in = hb.base; Lv.in_cs = hb.cs; Lv.in_coff = 0; Lv.vin = 1;
        if (x3_vin_ok(Lv, cus, sw) && !(rgb_layer(c) && x3_rgb_fits(L))) L = Lv;
        else st.late_pool = vin_buf;   // no variant: the pool after all
        vin_buf = -1;
      }
      const bool perm = k == perm_op || (perm_op != (size_t)-1 && k == perm_op + 1);
      int kind = PK_X3;
      if (perm && k == perm_op) {
        // Mconv6 of the pair's two launches: output channels in the fused K order, its K
        // summed in one sequence as the fused kernel does (no ranges)
        kind = PK_X3P; L.bias = c.param(PB_BIAS_PERM); L.slope = c.param(PB_SLOPE_PERM);
        L.allow_split = 0;
      } else if (perm) {
        kind = PK_X3P;   // Mconv7 reading them through that channel map
      } else if (c.x3_wide) {   // 256-channel tiles, two pairs per step, where the grid is big enough
        ConvLaunch Lw = L;
        Lw.bco = 256;
        if (x3_wide1(Lw, cus, sw)) { L.bco = 256; kind = PK_X3_WIDE; }
      }
      L.wx3 = c.pack(kind, h16);
      if (h16) L.f16 = 1;
      if (a16) store16(L, k);
      // the next op pools this conv's output: write pair maxima to its half-width buffer
      if (k + 1 < nops && net->ops[k + 1].type == 1 && net->ops[k + 1].in == op.out && op.out_coff == 0 &&
          net->ops[k + 1].C == c.cout && fuse_pools && x3_hpool_ok(L, cus, sw)) {
        const Act& hb = act[net->ops[k + 1].hbuf];
        L.out = hb.base; L.out_pad = 0; L.out_cs = hb.cs; L.out_coff = 0;
        L.hpool = 1;
        fused = true;
      }
      // the Winograd kernel: plain 3x3 launches -- no pool on either side (decided from the graph,
      // not from whether the pool is fused, so the pool switches never change a conv's arithmetic),
      // no fold, no K ranges
      const bool pool_side = (k > 0 && net->ops[k - 1].type == 1 && net->ops[k - 1].out == op.in) ||
                             (k + 1 < nops && net->ops[k + 1].type == 1 && net->ops[k + 1].in == op.out);
      const bool folds = far && (far->fold_ws_off[k] >= 0 || far->fold_tab_off[k] >= 0);
      ConvLaunch Lw = L;
      Lw.wx3 = c.pack(PK_WINO_F16);
      Lw.wscale_inv = c.inv[PK_WINO_F16];
      if (!h16 && !perm && !pool_side && w2_enabled(sw, L) && owns_pack(c, PK_WINO_F16) && !L.vin && !L.hpool && !folds &&
          x3_split_ranges(L, nullptr, cus, sw) <= 1 && wino_f16_fits(Lw)) {
        L = Lw;
        st.kind = Step::W2;
        st.code[0] = x3_variant_code(X3V_W2, 3, 128, 64);
      } else if (rgb_layer(c) && x3_rgb_fits(L) && rgb_kernel_enabled(sw) && !L.vin) {
        L.wx3 = c.pack(PK_RGB, h16);
        st.kind = Step::X3_RGB;
        st.choice = x3_choose_rgb(L);
        st.code[0] = st.choice.code;
        st.covered = true;
      } else {
        // (the net input is fp32 in every arena: only the 3-channel kernel reads it)
        st.kind = Step::X3;
        st.choice = x3_choose(L, cus, sw);
        st.code[0] = st.choice.code;
        st.covered = !folds && op.in != net->in_buf && st.choice.act16;
      }
    } else {
      st.kind = Step::DIRECT;
    }
    if (vin_buf >= 0) st.error = "pooled-input staging: the conv after a skipped pool did not take it";
  }
  return steps;
}

// ISL_ACT_FP16 is all or nothing per run: whether every step of a one-term run on the geometry
// `geo` (no addresses) has an fp16-storage form.  A conv off the x3 kernels, a fold plan or K
// ranges across blocks (split-K, the wave-range kernel: the latency-bound small grids) send the
// whole run to an fp32 arena.
static bool act16_plan_ok(const isl_net* net, const std::vector<Act>& geo) {
  if (fold_enabled()) return false;
#ifdef ISLPOSE_DEV
  if (x3_wino_enabled(x3_switches())) return false;
#endif
  for (const Step& st : plan_steps(net, geo, true, true, nullptr))
    if (!st.covered) return false;
  return true;
}

// Split-K fold plan of the current arena at its batch size (small grids, e.g. batch-1
// Mode R frames, where every 23x41 stage layer splits its canonical K ranges across
// blocks): a producer whose output slice is read only by convs on the generic loop -- no
// net output, no pool, cout a multiple of 8 -- keeps its partial sums in a region of its
// own and skips its reduce launch; each consumer's X3Fold table points its chunks at them.
// Same bits: the consumer's staging performs the reduce's arithmetic.
static int plan_fold(isl_net* net, hipStream_t s) {
  isl_net::Arena& ar = *net->cur;
  // the plan depends on the batch size and on the K-range mode (which layers split)
  const int mode = (net->algo == ISL_ALGO_X3 && fold_enabled()) ? net->split_k : 0;
  if (ar.fold_n == net->pn && ar.fold_mode == mode) return ISL_OK;
  const size_t nops = net->ops.size();
  ar.fold_ws_off.assign(nops, -1);
  ar.fold_tab_off.assign(nops, -1);
  ar.fold_n = net->pn;
  ar.fold_mode = mode;
  if (!mode) return ISL_OK;
  const X3Switches fsw = x3_switches();
  auto is_conv_x3 = [&](size_t k) { return net->ops[k].type == 0 && x3_fits(basic_launch(net, net->act, net->ops[k])); };
  // a consumer may fold only on the generic loop with no pool on either side
  auto consumer_ok = [&](size_t j) {
    if (!is_conv_x3(j)) return false;
    const Op& op = net->ops[j];
    if (j > 0 && net->ops[j - 1].type == 1 && net->ops[j - 1].out == op.in) return false;
    if (j + 1 < nops && net->ops[j + 1].type == 1 && net->ops[j + 1].in == op.out) return false;
    const ConvLayer& c = net->layers[op.layer];
    if (rgb_layer(c)) return false;
    return x3_fold_ok(basic_launch(net, net->act, op), device_cus(), fsw);
  };
  struct Prod { size_t k; int S; long long off; std::vector<size_t> cons; };
  std::vector<Prod> prods;
  long long total = 0;
  for (size_t k = 0; k < nops; ++k) {
    const Op& op = net->ops[k];
    if (!is_conv_x3(k)) continue;
    const ConvLayer& c = net->layers[op.layer];
    if (c.cout % 8 || rgb_layer(c)) continue;
    ConvLaunch L = basic_launch(net, net->act, op);
    bool across = false;
    const int S = x3_split_ranges(L, &across, device_cus(), fsw);
    if (S < 2 || !across) continue;
    const int lo = op.out_coff, hi = op.out_coff + c.cout;
    auto overlaps = [&](const OutRef& o) { return o.buf == op.out && o.coff < hi && o.coff + o.C > lo; };
    if (overlaps(net->out0) || (net->n_out > 1 && overlaps(net->out1))) continue;
    bool ok = true;
    std::vector<size_t> cons;
    for (size_t j = k + 1; j < nops && ok; ++j) {
      const Op& oj = net->ops[j];
      if (oj.type == 1) {   // a pool reading the slice
        if (oj.in == op.out) ok = false;
        if (oj.out == op.out) break;
        continue;
      }
      const ConvLayer& cj = net->layers[oj.layer];
      if (oj.in == op.out && oj.in_coff < hi && oj.in_coff + cj.cin_phys > lo) {
        if (consumer_ok(j)) cons.push_back(j);
        else ok = false;
      }
      if (oj.out == op.out && oj.out_coff < hi && oj.out_coff + cj.cout > lo) break;   // overwritten
    }
    if (!ok || cons.empty()) continue;
    const long long floats = (long long)S * L.n * ((c.cout + 7) / 8) * 8 * L.H * L.W;
    prods.push_back({k, S, total, cons});
    total += (floats + 63) / 64 * 64;
  }
  if (prods.empty()) return ISL_OK;
  if ((size_t)total > ar.fold_mem_floats) {
    if (ar.fold_mem) HIP_OK(hipFree(ar.fold_mem));   // waits for queued work that may still read it
    ar.fold_mem = nullptr;
    ar.fold_mem_floats = 0;
    HIP_OK(hipMalloc(&ar.fold_mem, (size_t)total * sizeof(float)));
    ar.fold_mem_floats = (size_t)total;
  }
  // consumer tables: one X3Fold per input chunk of every consumer
  std::vector<X3Fold> tab;
  std::map<size_t, long long> cons_off;
  for (const Prod& p : prods)
    for (size_t j : p.cons)
      if (!cons_off.count(j)) {
        cons_off[j] = (long long)tab.size();
        const ConvLayer& cj = net->layers[net->ops[j].layer];
        tab.resize(tab.size() + cj.cin_phys / 8, X3Fold{nullptr, 0, 0, nullptr, nullptr, 1.f, 0, 0, 0});
      }
  for (const Prod& p : prods) {
    const Op& op = net->ops[p.k];
    const ConvLayer& c = net->layers[op.layer];
    const Act& o = net->act[op.out];
    const long long plane = (long long)o.H * o.W * 8, c8 = (c.cout + 7) / 8;
    ar.fold_ws_off[p.k] = p.off;
    for (size_t j : p.cons) {
      const Op& oj = net->ops[j];
      const ConvLayer& cj = net->layers[oj.layer];
      for (int ch = 0; ch < cj.cin_phys / 8; ++ch) {
        const int pc = oj.in_coff + 8 * ch;              // physical channel of the buffer
        if (pc < op.out_coff || pc >= op.out_coff + c.cout) continue;
        const int cc = (pc - op.out_coff) / 8;           // the producer's chunk
        X3Fold& f = tab[cons_off[j] + ch];
        f.ws = ar.fold_mem + p.off + cc * plane;
        f.fstride = c8 * plane;
        f.sstride = (long long)o.n * c8 * plane;
        f.bias = c.param(PB_BIAS) + cc * 8;
        f.slope = c.act == ACT_PRELU ? c.param(PB_SLOPE) + cc * 8 : nullptr;
        f.scale = c.inv[PK_X3];
        f.S = p.S;
        f.act = c.act;
      }
    }
  }
  for (auto& kv : cons_off) ar.fold_tab_off[kv.first] = kv.second;
  if (tab.size() > ar.fold_tab_n) {
    if (ar.fold_tab) HIP_OK(hipFree(ar.fold_tab));
    ar.fold_tab = nullptr;
    ar.fold_tab_n = 0;
    HIP_OK(hipMalloc(&ar.fold_tab, tab.size() * sizeof(X3Fold)));
    ar.fold_tab_n = tab.size();
  }
  // stream-ordered: a run queued before on this stream has read the old table (same arena,
  // same stream); the host vector is staged by HIP before the call returns
  HIP_OK(hipMemcpyAsync(ar.fold_tab, tab.data(), tab.size() * sizeof(X3Fold), hipMemcpyHostToDevice, s));
  return ISL_OK;
}

// The timing record of a step that has run: kind (isl_net_timing's op kinds: 0 no conv, 1 fp32
// direct, 2 fp32 Winograd, 3 split-fp16 direct, 4 wino_x3, 5 wino_f16), FLOPs and MFMA FLOPs on
// its first op, and one event per covered op -- the ops a launch swallowed are empty intervals.
static int record_step(const isl_net* net, isl_net::TimedRun* tr, const Step& st, hipStream_t s) {
  const ConvLaunch& L = st.L;
  int kind = 3;
  double mf = 0.0, macs = 0.0;   // macs: per output pixel, over the convs the step covers
  switch (st.kind) {
    case Step::POOL: case Step::VPOOL: case Step::POOL_DEFERRED: kind = 0; break;
#ifdef ISLPOSE_DEV
    case Step::WINO_X3: kind = 4; mf = wino_x3_mfma_flops(L); break;
#endif
    case Step::DIRECT: kind = 1; mf = conv_mfma_flops(L); break;
    case Step::WINO: kind = 2; mf = wino_mfma_flops(L); break;
    case Step::X3: case Step::X3_RGB: case Step::PAIR: mf = st.choice.mfma_flops; break;
    case Step::W2: kind = 5; mf = wino_f16_mfma_flops(L); break;
    case Step::C12: mf = conv_x3_c12_mfma_flops(L); break;
  }
  for (int j = 0; j < st.nops; ++j) {
    const Op& o = net->ops[st.op + j];
    if (o.type != 0) continue;
    const ConvLayer& c = net->layers[o.layer];
    macs += (double)c.cout * c.cin * c.k * c.k;
  }
  for (int j = 0; j < st.nops; ++j) {
    tr->kind.push_back(j ? 0 : kind);
    tr->flops.push_back(j ? 0.0 : 2.0 * macs * L.H * L.W * L.n);
    tr->mfma_flops.push_back(j ? 0.0 : mf);
    HIP_OK(hipEventRecord(tr->ev[st.op + j + 1], s));
  }
  return ISL_OK;
}

// One eager run of the conv chain: the launch plan (plan_steps), issued step by step.
static int run_ops_eager(isl_net* net, hipStream_t s) {
  isl_net::TimedRun* tr = nullptr;
  if (net->timing) {
    net->timed.emplace_back();
    tr = &net->timed.back();
    tr->ev.resize(net->ops.size() + 1);
    for (hipEvent_t& e : tr->ev) HIP_OK(hipEventCreate(&e));
    HIP_OK(hipEventRecord(tr->ev[0], s));
  }
  net->op_variant.assign(net->ops.size(), 0);
  if (const int rc = plan_fold(net, s)) return rc;
  isl_net::Arena& ar = *net->cur;
  const bool h16 = net->algo == ISL_ALGO_X3 && net->precision == ISL_PREC_FP16;
  if (h16 && !net->packed_hi) return fail(ISL_E_STATE, "fp16 precision: hi-only filters not uploaded");
  // ISL_ACT_FP16: the arena of this plan holds fp16 between the convs (plan() found every step covered)
  const bool a16 = ar.a16;
  if (a16 && !h16) return fail(ISL_E_STATE, "fp16 activation storage: the arena of this plan needs ISL_ALGO_X3 with ISL_PREC_FP16");
  X3Switches sw;
  std::vector<Step> steps = plan_steps(net, net->act, h16, a16, &ar, &sw);
  for (Step& st : steps) {
    const size_t k = st.op;
    const Op& op = net->ops[k];
    ConvLaunch& L = st.L;
    if (st.error) return fail(ISL_E_STATE, st.error);
    if (a16 && st.kind >= Step::DIRECT) return fail(ISL_E_STATE, "fp16 activation storage: a conv off the x3 kernels");
    if (st.late_pool >= 0) {
      const Op& pool = net->ops[st.late_pool];
      HIP_OK(launch_vpool2(net->act[pool.hbuf], net->act[pool.out], pool.C, s));
      net->op_variant[st.late_pool] = 0;
    }
    if (st.kind == Step::X3) {
      // the split-K workspace and the fold pointers: allocations of this arena
      if (ar.fold_ws_off[k] >= 0 || ar.fold_tab_off[k] >= 0) {
        // a fold producer keeps its partial sums, a fold consumer reads such: another kernel
        if (ar.fold_ws_off[k] >= 0) L.fold_out = 1;
        if (ar.fold_tab_off[k] >= 0) {
          if (L.vin || L.hpool || !x3_fold_ok(L, device_cus(), sw)) return fail(ISL_E_STATE, "split-K fold: consumer off the generic loop");
          L.fold = ar.fold_tab + ar.fold_tab_off[k];
        }
        st.choice = x3_choose(L, device_cus(), sw);
        st.code[0] = st.choice.code;
      }
      const size_t need = st.choice.ws_floats;
      if (need > ar.ks_floats) {
        if (net->capturing) return fail(ISL_E_STATE, "graph capture: split-K workspace growth");
        drop_graphs(ar);   // they name the old workspace
        // grow-only; hipFree waits for the queued work that may still read the old one
        if (ar.ks) HIP_OK(hipFree(ar.ks));
        ar.ks = nullptr;
        ar.ks_floats = 0;
        HIP_OK(hipMalloc(&ar.ks, need * sizeof(float)));
        ar.ks_floats = need;
      }
      L.ws = ar.ks;
      L.ws_floats = ar.ks_floats;
      if (L.fold_out) {   // a fold producer: its own partial-sum region, no reduce
        L.ws = ar.fold_mem + ar.fold_ws_off[k];
        L.ws_floats = need;
      }
    }
    for (int j = 0; j < st.nops; ++j) net->op_variant[k + j] = st.code[j];
    if (L.fold_out) net->op_variant[k] |= X3V_FOLD_OUT;
    switch (st.kind) {
      case Step::POOL: HIP_OK(launch_maxpool2(net->act[op.in], net->act[op.out], op.C, s)); break;
      case Step::VPOOL: HIP_OK(launch_vpool2(net->act[op.hbuf], net->act[op.out], op.C, s)); break;
      case Step::POOL_DEFERRED: break;
      case Step::WINO: HIP_OK(launch_wino(L, s)); break;
      case Step::W2: HIP_OK(launch_wino_f16(L, s)); break;
      case Step::C12: HIP_OK(launch_conv_x3_c12(L, st.L2, s)); break;
      case Step::X3_RGB: HIP_OK(launch_conv_x3_rgb(L, s)); break;
      case Step::X3: case Step::PAIR: HIP_OK(launch_conv_x3(L, st.choice, sw, s)); break;
      case Step::DIRECT: HIP_OK(launch_conv(L, s)); break;
#ifdef ISLPOSE_DEV
      case Step::WINO_X3: HIP_OK(launch_wino_x3(L, s)); break;
#endif
    }
    if (tr)
      if (const int rc = record_step(net, tr, st, s)) return rc;
  }
  return ISL_OK;
}

// Graph replay of the conv chain.  At batch 1 (Mode R, the reference's per-frame calls) the
// host enqueue of ~230 launches (selection logic + hipLaunchKernel, ~7.6 us each) took as
// long as the GPU work, so the GPU waited on the host (tools/b1_host.py).  A run key fixes
// everything the launches depend on besides the arena: batch size, K-range mode, algorithm
// and the ISLPOSE_* switches read per launch.  The first run of a key is eager (it sizes the
// workspaces), the second captures the chain on a private stream, instantiates it and
// launches it on the caller's stream; later runs replay it.  The kernels, their order and
// arguments are those of the eager run: the same bits.  Timed runs (isl_net_set_timing) and
// the split-K fold (its plan uploads a table) stay eager.
// The switches the launch selection of this build reads (x3_switch_table: its run_key rows), in
// table order, each hashed as name=value; -- so the key depends on their values only, not on the
// order of environ or on unrelated ISLPOSE_* variables.
static unsigned long long run_key(const isl_net* net) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](unsigned long long v) { h = (h ^ v) * 1099511628211ull; };
  mix((unsigned long long)net->pn);
  mix((unsigned long long)net->split_k + 16 * (unsigned long long)net->algo + 256 * (unsigned long long)net->precision +
      4096 * (unsigned long long)(net->cur && net->cur->a16 ? 1 : 0));
  int nsw = 0;
  const X3SwitchDef* defs = x3_switch_table(&nsw);
  for (int i = 0; i < nsw; ++i) {
    if (!defs[i].run_key) continue;
    const char* name = defs[i].name;
    const char* v = getenv(name);
    for (const char* c = name; *c; ++c) mix((unsigned char)*c);
    mix('=');
    if (v)
      for (const char* c = v; *c; ++c) mix((unsigned char)*c);
    else
      mix(0x100);   // unset differs from set-but-empty
    mix(';');
  }
  return h;
}

// instantiated graphs kept per arena (least recently launched dropped beyond it): ragged hand
// crop batches and A/B switches would otherwise add executables without bound
constexpr size_t kGraphsPerArena = 8;
constexpr size_t kGraphSeenCap = 64;

static bool graph_enabled(const isl_net* net) {
  const char* e = getenv("ISLPOSE_NET_GRAPH");
  const bool on = e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : net->graph != 0;
  return on && !net->timing && !fold_enabled();
}

// An event behind the latest work on stream s that may write the range flag / trip count
// (isl_net_check and isl_net_range_info wait for these instead of draining the device).
static int note_flag_stream(isl_net* net, hipStream_t s) {
  if (net->flag_events.size() >= 16 && !net->flag_events.count(s)) {
    // many distinct streams (rare): wait for the recorded work and start over
    for (auto& kv : net->flag_events) {
      HIP_OK(hipEventSynchronize(kv.second));
      HIP_OK(hipEventDestroy(kv.second));
    }
    net->flag_events.clear();
  }
  hipEvent_t& e = net->flag_events[s];
  if (!e) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_OK(hipEventRecord(e, s));
  return ISL_OK;
}

static int wait_flag_streams(isl_net* net) {
  for (auto& kv : net->flag_events) HIP_OK(hipEventSynchronize(kv.second));
  return ISL_OK;
}

static int run_ops_graph(isl_net* net, hipStream_t s);
static int run_ops(isl_net* net, hipStream_t s) {
  const int rc = graph_enabled(net) ? run_ops_graph(net, s) : run_ops_eager(net, s);
  if (rc) return rc;
  return note_flag_stream(net, s);
}

static int run_ops_graph(isl_net* net, hipStream_t s) {
  isl_net::Arena& ar = *net->cur;
  const unsigned long long key = run_key(net);
  if (!ar.graph_retired.empty()) {
    const int rc = reap_graphs(ar);
    if (rc) return rc;
  }
  // after a replay, the event its eviction would wait for
  auto launch = [&](isl_net::Arena::Graph& G) -> int {
    HIP_OK(hipGraphLaunch(G.exec, s));
    if (!G.done) HIP_OK(hipEventCreateWithFlags(&G.done, hipEventDisableTiming));
    HIP_OK(hipEventRecord(G.done, s));
    return ISL_OK;
  };
  auto g = ar.graphs.find(key);
  if (g != ar.graphs.end()) {
    net->op_variant = g->second.op_variant;
    g->second.last_use = ++ar.graph_clock;
    return launch(g->second);
  }
  if (ar.graph_failed.count(key)) return run_ops_eager(net, s);
  if (ar.graph_seen.size() >= kGraphSeenCap && !ar.graph_seen.count(key)) ar.graph_seen.clear();
  int& seen = ar.graph_seen[key];
  if (seen++ < 1) return run_ops_eager(net, s);
  if (!net->cap_stream) HIP_OK(hipStreamCreateWithFlags(&net->cap_stream, hipStreamNonBlocking));
  HIP_OK(hipStreamBeginCapture(net->cap_stream, hipStreamCaptureModeRelaxed));
  net->capturing = true;
  const int rc = run_ops_eager(net, net->cap_stream);
  net->capturing = false;
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(net->cap_stream, &graph);
  hipGraphExec_t exec = nullptr;
  hipError_t ei = hipErrorUnknown;
  if (rc == ISL_OK && ec == hipSuccess && graph) ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (rc != ISL_OK || ec != hipSuccess || ei != hipSuccess) {
    // nothing ran: the chain was only recorded.  Run it eagerly, and keep this key eager
    (void)hipGetLastError();
    if (exec) (void)hipGraphExecDestroy(exec);
    ar.graph_failed.insert(key);   // kept apart from graph_seen, whose cap clears it
    ar.graph_seen.erase(key);
    return run_ops_eager(net, s);
  }
  while (ar.graphs.size() >= kGraphsPerArena) {
    auto lru = ar.graphs.begin();
    for (auto j = ar.graphs.begin(); j != ar.graphs.end(); ++j)
      if (j->second.last_use < lru->second.last_use) lru = j;
    ar.graph_retired.push_back(lru->second);
    ar.graphs.erase(lru);
  }
  isl_net::Arena::Graph& G = ar.graphs[key];
  G.exec = exec;
  G.op_variant = net->op_variant;
  G.last_use = ++ar.graph_clock;
  return launch(G);
}

// Net output `which` of the current plan: its slice of the stage buffers, or (an fp16-storage
// arena) the fp32 buffer of its own that the last layer writing it also stores to
static OutRef out_ref(const isl_net* net, int which) {
  const OutRef& o = which == 0 ? net->out0 : net->out1;
  if (net->cur && net->cur->a16) return OutRef{net->out32_buf[which], 0, o.C};
  return o;
}

static int copy_outputs(isl_net* net, float* d_out0, float* d_out1, hipStream_t s) {
  const OutRef o0 = out_ref(net, 0);
  if (d_out0) HIP_OK(launch_unpack_nchw(net->act[o0.buf], o0.coff, o0.C, d_out0, s));
  if (d_out1 && net->n_out > 1) {
    const OutRef o1 = out_ref(net, 1);
    HIP_OK(launch_unpack_nchw(net->act[o1.buf], o1.coff, o1.C, d_out1, s));
  }
  return ISL_OK;
}

int net_kind(const isl_net* net) { return net->kind; }
int net_device(const isl_net* net) { return net->device; }

int net_low_res(isl_net* net, int which, MapSrc* m) {
  if (!net->arena) return fail(ISL_E_STATE, "no network output in the arena (run the net first)");
  const OutRef o = out_ref(net, which);
  const Act& a = net->act[o.buf];
  if (a.esize != 4) return fail(ISL_E_STATE, "network output buffer is not fp32");
  const int Wp = a.W + 2 * a.pad;
  if (o.coff % 8) return fail(ISL_E_STATE, "network output slice not on a chunk");
  m->base = a.base + (size_t)(o.coff / 8) * a.chunk_elems() + ((size_t)a.pad * Wp + a.pad) * 8;
  m->xs = 8; m->ys = (long long)Wp * 8; m->cstr = 1; m->fs = (long long)a.frame_elems();
  m->cshift = 3; m->cbig = (long long)a.chunk_elems();
  m->sh = a.H; m->sw = a.W;
  return ISL_OK;
}

void* net_scratch(isl_net* net, size_t bytes) {
  if (bytes <= net->scratch_bytes) return net->scratch;
  if (net->scratch) { (void)hipFree(net->scratch); net->scratch = nullptr; net->scratch_bytes = 0; }
  hipError_t e = hipMalloc(&net->scratch, bytes);
  if (e != hipSuccess) { set_error(std::string("scratch hipMalloc: ") + hipGetErrorString(e)); return nullptr; }
  net->scratch_bytes = bytes;
  return net->scratch;
}

size_t net_scratch_size(const isl_net* net) { return net->scratch_bytes; }

PostLanes* net_post_lanes(isl_net* net) {
  if (net->lanes) return net->lanes;
  PostLanes* L = new PostLanes();
  L->mid = nullptr;
  L->mid_bytes = 0;
  L->mid_used = false;
  hipError_t e = hipEventCreateWithFlags(&L->fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&L->mid_free, hipEventDisableTiming);
  for (int k = 0; k < ISL_POST_LANES && e == hipSuccess; ++k) {
    L->scratch[k] = nullptr;
    L->bytes[k] = 0;
    e = hipStreamCreateWithFlags(&L->stream[k], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L->join[k], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    set_error(std::string("post lanes: ") + hipGetErrorString(e));
    delete L;   // (a partial set of streams/events is leaked on this failure path only)
    return nullptr;
  }
  net->lanes = L;
  return L;
}

}  // namespace isl

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

int isl_abi_version(void) { return ISL_ABI_VERSION; }
const char* isl_last_error(void) { return isl::g_err.c_str(); }

int isl_net_create(int kind, int device, isl_net** out) {
  if (!out) return fail(ISL_E_ARG, "out is NULL");
  *out = nullptr;
  if (kind < ISL_BODY25 || kind > ISL_HAND) return fail(ISL_E_ARG, "unknown net kind");
  isl_net* net = new isl_net();
  net->kind = kind;
  net->device = device;
  net->algo = default_algo();
  net->precision = default_precision();
  net->act_storage = default_act_storage();
  {
    // K-range mode (isl_net_set_split_k): 1 canonical ranges (default), 0 none, 2 latency
    const char* e = getenv("ISLPOSE_X3_SPLITK");
    net->split_k = e && (e[0] == '0' || e[0] == '2') ? e[0] - '0' : 1;
  }
  net->layers = kind == ISL_BODY25 ? body25_layers() : kind == ISL_COCO ? coco_layers() : hand_layers();
  for (size_t i = 0; i < net->layers.size(); ++i) {
    const ConvLayer& c = net->layers[i];
    net->layer_index[c.name] = (int)i;
    net->params.push_back({c.name + ".weight", (int64_t)c.cout * c.cin * c.k * c.k});
    net->params.push_back({c.name + ".bias", (int64_t)c.cout});
    if (c.act == ACT_PRELU) net->params.push_back({c.prelu + ".weight", (int64_t)c.cout});
  }
  if (kind == ISL_BODY25) build_body25(net);
  else if (kind == ISL_COCO) build_coco(net);
  else build_hand(net);
  plan_fuse67(net);
  // ISL_ACT_FP16: an fp32 buffer per net output (allocated in fp16-storage arenas only), and
  // the last op that writes the output
  for (int o = 0; o < net->n_out; ++o) {
    const OutRef& r = o == 0 ? net->out0 : net->out1;
    net->bufs.push_back({net->bufs[r.buf].level, round8(r.C), net->bufs[r.buf].pad, 0, 1});
    net->out32_buf[o] = (int)net->bufs.size() - 1;
    for (size_t k = 0; k < net->ops.size(); ++k)
      if (net->ops[k].type == 0 && net->ops[k].out == r.buf && net->ops[k].out_coff == r.coff) net->out_op[o] = (int)k;
  }
  *out = net;
  return ISL_OK;
}

int isl_net_destroy(isl_net* net) {
  if (!net) return ISL_OK;
  (void)hipSetDevice(net->device);
  for (ConvLayer& c : net->layers) {
    for (auto& forms : c.dev)
      for (DevBuf& d : forms)
        if (d.p) (void)hipFree(d.p);
    for (DevBuf& d : c.par)
      if (d.p) (void)hipFree(d.p);
  }
  for (auto& kv : net->flag_events) {
    (void)hipEventSynchronize(kv.second);
    (void)hipEventDestroy(kv.second);
  }
  net->flag_events.clear();
  if (net->d_flag) (void)hipFree(net->d_flag);
  if (net->d_trips) (void)hipFree(net->d_trips);
  drop_all_graphs(net);
  if (net->cap_stream) (void)hipStreamDestroy(net->cap_stream);
  for (auto& kv : net->plans) {
    if (kv.second.tab_ev) {
      (void)hipEventSynchronize(kv.second.tab_ev);
      (void)hipEventDestroy(kv.second.tab_ev);
    }
    if (kv.second.tab_pin) (void)hipHostFree(kv.second.tab_pin);
    if (kv.second.tab) (void)hipFree(kv.second.tab);
    if (kv.second.ks) (void)hipFree(kv.second.ks);
    if (kv.second.fold_mem) (void)hipFree(kv.second.fold_mem);
    if (kv.second.fold_tab) (void)hipFree(kv.second.fold_tab);
  }
  for (auto& kv : net->plans) (void)hipFree(kv.second.base);
  if (net->scratch) (void)hipFree(net->scratch);
  if (net->lanes) {
    for (int k = 0; k < ISL_POST_LANES; ++k) {
      (void)hipStreamSynchronize(net->lanes->stream[k]);
      if (net->lanes->scratch[k]) (void)hipFree(net->lanes->scratch[k]);
      (void)hipStreamDestroy(net->lanes->stream[k]);
      (void)hipEventDestroy(net->lanes->join[k]);
    }
    (void)hipEventDestroy(net->lanes->fork);
    if (net->lanes->mid) {
      (void)hipEventSynchronize(net->lanes->mid_free);
      (void)hipFree(net->lanes->mid);
    }
    (void)hipEventDestroy(net->lanes->mid_free);
    delete net->lanes;
  }

  for (auto& r : net->timed)
    for (hipEvent_t e : r.ev) (void)hipEventDestroy(e);
  delete net;
  return ISL_OK;
}

int isl_net_param_count(const isl_net* net) { return net ? (int)net->params.size() : fail(ISL_E_ARG, "net is NULL"); }

int isl_net_param_info(const isl_net* net, int index, const char** name, int64_t* numel) {
  if (!net || index < 0 || index >= (int)net->params.size()) return fail(ISL_E_ARG, "bad parameter index");
  if (name) *name = net->params[index].first.c_str();
  if (numel) *numel = net->params[index].second;
  return ISL_OK;
}

int isl_net_set_param(isl_net* net, const char* caffe_name, const float* host, int64_t numel) {
  if (!net || !caffe_name || !host) return fail(ISL_E_ARG, "NULL argument");
  std::string nm(caffe_name);
  const size_t dot = nm.rfind('.');
  if (dot == std::string::npos || (nm.substr(dot) != ".weight" && nm.substr(dot) != ".bias"))
    return fail(ISL_E_PARAM, nm);
  const std::string base = nm.substr(0, dot), field = nm.substr(dot + 1);
  for (ConvLayer& c : net->layers) {
    std::vector<float>* dst = nullptr;
    bool* flag = nullptr;
    int64_t want = 0;
    if (c.name == base && field == "weight") { dst = &c.w; flag = &c.has_w; want = (int64_t)c.cout * c.cin * c.k * c.k; }
    else if (c.name == base && field == "bias") { dst = &c.b; flag = &c.has_b; want = c.cout; }
    else if (!c.prelu.empty() && c.prelu == base && field == "weight") { dst = &c.s; flag = &c.has_s; want = c.cout; }
    if (!dst) continue;
    if (numel != want)
      return fail(ISL_E_PARAM, nm + ": expected " + std::to_string(want) + " elements, got " + std::to_string(numel));
    dst->assign(host, host + numel);
    *flag = true;
    net->packed = false;
    return ISL_OK;
  }
  return fail(ISL_E_PARAM, nm);
}

static int prepare(isl_net* net) {
  HIP_OK(hipSetDevice(net->device));
  if (!net->packed) {
    const int rc = upload_params(net);
    if (rc) return rc;
  }
  if (net->precision == ISL_PREC_FP16 && net->algo == ISL_ALGO_X3 && !net->packed_hi) return upload_hi_packs(net);
  return ISL_OK;
}

int isl_net_forward(isl_net* net, const float* d_x, int n, int h, int w, float* d_out0, float* d_out1, void* stream) {
  if (!net || !d_x || !d_out0) return fail(ISL_E_ARG, "NULL argument");
  if (net->n_out == 1 && d_out1) return fail(ISL_E_ARG, "hand net has a single output");
  if (net->n_out == 2 && !d_out1) return fail(ISL_E_ARG, "body nets have two outputs");
  int rc = prepare(net);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = plan(net, n, h, w, s))) return rc;
  // the split-fp16 convs take |x| < 65504: the pack raises the range flag for anything else in the
  // caller's tensor (the fp32 kernels of the fallback take every value and raise nothing)
  HIP_OK(launch_pack_nchw(d_x, n, 3, h, w, net->act[net->in_buf], net->algo == ISL_ALGO_X3 ? net->d_flag : nullptr, s));
  if ((rc = run_ops(net, s))) return rc;
  return copy_outputs(net, d_out0, d_out1, s);
}

// Upload the image table built in net->h_tab (stream-ordered; pageable source is staged by HIP).
// The table lives with the current plan's arena (one per net size).
static int upload_tab(isl_net* net, hipStream_t s) {
  const size_t bytes = net->h_tab.size();
  isl_net::Arena& ar = *net->cur;
  // the same frames geometry as the last upload into this arena's table (per-frame callers,
  // a video's batches): the device copy already holds it.  Only upload_tab writes it, in
  // stream order, so skipping the pageable copy (a blit plus a host-side stall) is safe
  if (ar.tab && ar.tab_host == net->h_tab) {
    net->d_tab = ar.tab;
    return ISL_OK;
  }
  if (bytes > ar.tab_bytes) {
    if (ar.tab) HIP_OK(hipFree(ar.tab));
    ar.tab = nullptr;
    ar.tab_bytes = 0;
    HIP_OK(hipMalloc(&ar.tab, bytes));
    ar.tab_bytes = bytes;
  }
  // through a pinned staging buffer, so the call never waits for the stream (the hand scales'
  // crop tables change every frame, and each scale's stream must not block the host enqueue of
  // the next): the previous copy out of the staging buffer has long completed, normally
  if (ar.tab_ev) HIP_OK(hipEventSynchronize(ar.tab_ev));
  if (bytes > ar.tab_pin_bytes) {
    if (ar.tab_pin) HIP_OK(hipHostFree(ar.tab_pin));
    ar.tab_pin = nullptr;
    ar.tab_pin_bytes = 0;
    HIP_OK(hipHostMalloc(&ar.tab_pin, bytes, hipHostMallocDefault));
    ar.tab_pin_bytes = bytes;
  }
  memcpy(ar.tab_pin, net->h_tab.data(), bytes);
  HIP_OK(hipMemcpyAsync(ar.tab, ar.tab_pin, bytes, hipMemcpyHostToDevice, s));
  if (!ar.tab_ev) HIP_OK(hipEventCreateWithFlags(&ar.tab_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(ar.tab_ev, s));
  ar.tab_host = net->h_tab;
  net->d_tab = ar.tab;
  return ISL_OK;
}

int isl_net_preprocess(isl_net* net, const uint8_t* d_frames, int n, int H, int W, double scale, int* net_h,
                       int* net_w, void* stream) {
  if (!net || !d_frames || n <= 0 || H <= 0 || W <= 0 || !(scale > 0)) return fail(ISL_E_ARG, "bad argument");
  // cv::resize dsize from fx/fy: saturate_cast<int>(W*fx) = cvRound (half to even)
  const int rh = (int)std::nearbyint(H * scale), rw = (int)std::nearbyint(W * scale);
  if (rh <= 0 || rw <= 0) return fail(ISL_E_ARG, "resized image is empty");
  const int ph = (rh + 7) / 8 * 8, pw = (rw + 7) / 8 * 8;  // padRightDownCorner (util.py:12-32)
  int rc = prepare(net);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = plan(net, n, ph, pw, s))) return rc;
  const size_t eb = preprocess_entry_bytes();
  net->h_tab.resize(eb * n);
  for (int f = 0; f < n; ++f)
    preprocess_entry(net->h_tab.data() + eb * f, (long long)f * H * W * 3, H, W, rh, rw, 1.0 / scale);
  if ((rc = upload_tab(net, s))) return rc;
  HIP_OK(launch_preprocess_tab(d_frames, (long long)W * 3, net->d_tab, n, net->act[net->in_buf], s));
  if (net_h) *net_h = ph;
  if (net_w) *net_w = pw;
  return ISL_OK;
}

int isl_net_preprocess_crops(isl_net* net, const uint8_t* d_frames, int n_frames, int H, int W,
                             const isl_crop* crops, int n_crops, double scale_times_box, int* net_h, int* net_w,
                             void* stream) {
  return isl_net_preprocess_crops_flip(net, d_frames, n_frames, H, W, crops, nullptr, n_crops, scale_times_box, net_h,
                                       net_w, stream);
}

int isl_net_preprocess_crops_flip(isl_net* net, const uint8_t* d_frames, int n_frames, int H, int W,
                                  const isl_crop* crops, const uint8_t* flip, int n_crops, double scale_times_box,
                                  int* net_h, int* net_w, void* stream) {
  if (!net || !d_frames || !crops || n_frames <= 0 || n_crops <= 0 || H <= 0 || W <= 0 || !(scale_times_box > 0))
    return fail(ISL_E_ARG, "bad argument");
  const size_t eb = preprocess_entry_bytes();
  net->h_tab.resize(eb * n_crops);
  int ph = 0, pw = 0;
  for (int i = 0; i < n_crops; ++i) {
    const isl_crop& c = crops[i];
    if (c.frame < 0 || c.frame >= n_frames || c.x < 0 || c.y < 0 || c.w <= 0 || c.h <= 0 || c.x + c.w > W ||
        c.y + c.h > H)
      return fail(ISL_E_ARG, "crop " + std::to_string(i) + " outside its frame");
    // Hand.__call__: scale = x * boxsize / oriImg.shape[0]; cv2.resize(fx=fy=scale) (hand.py:33-37)
    const double m = scale_times_box / c.h;
    const int rh = (int)std::nearbyint(c.h * m), rw = (int)std::nearbyint(c.w * m);
    if (rh <= 0 || rw <= 0) return fail(ISL_E_ARG, "resized crop is empty");
    const int h8 = (rh + 7) / 8 * 8, w8 = (rw + 7) / 8 * 8;
    if (i == 0) { ph = h8; pw = w8; }
    if (h8 != ph || w8 != pw) return fail(ISL_E_ARG, "crops resize to different net sizes: batch them separately");
    const long long off = (((long long)c.frame * H + c.y) * W + c.x) * 3;
    preprocess_entry(net->h_tab.data() + eb * i, off, c.h, c.w, rh, rw, 1.0 / m, flip && flip[i]);
  }
  int rc = prepare(net);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = plan(net, n_crops, ph, pw, s))) return rc;
  if ((rc = upload_tab(net, s))) return rc;
  HIP_OK(launch_preprocess_tab(d_frames, (long long)W * 3, net->d_tab, n_crops, net->act[net->in_buf], s));
  if (net_h) *net_h = ph;
  if (net_w) *net_w = pw;
  return ISL_OK;
}

int isl_net_debug_input(isl_net* net, float* d_x, void* stream) {
  if (!net || !net->arena || !d_x) return fail(ISL_E_STATE, "no input buffer yet");
  HIP_OK(hipSetDevice(net->device));
  HIP_OK(launch_unpack_nchw(net->act[net->in_buf], 0, 3, d_x, (hipStream_t)stream));
  return ISL_OK;
}

int isl_net_set_timing(isl_net* net, int on) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  net->timing = on != 0;
  return ISL_OK;
}

int isl_net_timing(isl_net* net, int max_ops, int* n_ops, int* n_runs, double* op_ms, int* op_kind,
                   double* op_flops, double* op_mfma_flops) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  const int nops = (int)net->ops.size();
  if (n_ops) *n_ops = nops;
  if (n_runs) *n_runs = (int)net->timed.size();
  if (!op_ms) return ISL_OK;   // query only
  if (max_ops < nops) return fail(ISL_E_ARG, "isl_net_timing: arrays shorter than the op count");
  HIP_OK(hipSetDevice(net->device));
  for (int k = 0; k < nops; ++k) {
    op_ms[k] = 0.0;
    if (op_kind) op_kind[k] = 0;
    if (op_flops) op_flops[k] = 0.0;
    if (op_mfma_flops) op_mfma_flops[k] = 0.0;
  }
  for (auto& r : net->timed) {
    HIP_OK(hipEventSynchronize(r.ev.back()));
    for (int k = 0; k < nops; ++k) {
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, r.ev[k], r.ev[k + 1]));
      op_ms[k] += ms;
      if (op_kind) op_kind[k] = r.kind[k];
      if (op_flops) op_flops[k] += r.flops[k];
      if (op_mfma_flops) op_mfma_flops[k] += r.mfma_flops[k];
    }
  }
  for (auto& r : net->timed)
    for (hipEvent_t e : r.ev) (void)hipEventDestroy(e);
  net->timed.clear();
  return ISL_OK;
}

int isl_net_op_info(const isl_net* net, int index, const char** name, int* variant) {
  if (!net || index < 0 || index >= (int)net->ops.size()) return fail(ISL_E_ARG, "bad op index");
  const Op& op = net->ops[index];
  if (name) *name = op.type == 1 ? "maxpool2" : net->layers[op.layer].name.c_str();
  if (variant) *variant = index < (int)net->op_variant.size() ? net->op_variant[index] : 0;
  return ISL_OK;
}

int isl_net_set_algo(isl_net* net, int algo) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (algo < ISL_ALGO_X3 || algo > ISL_ALGO_DIRECT) return fail(ISL_E_ARG, "unknown conv algorithm");
  net->algo = algo;
  return ISL_OK;
}

int isl_net_get_algo(const isl_net* net) { return net ? net->algo : fail(ISL_E_ARG, "net is NULL"); }

int isl_net_set_precision(isl_net* net, int precision) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (precision != ISL_PREC_FP32 && precision != ISL_PREC_FP16) return fail(ISL_E_ARG, "unknown precision");
  // (captured graphs are keyed by the precision, run_key: a switch re-keys them)
  net->precision = precision;
  return ISL_OK;
}

int isl_net_get_precision(const isl_net* net) { return net ? net->precision : fail(ISL_E_ARG, "net is NULL"); }

int isl_net_set_act_storage(isl_net* net, int storage) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (storage != ISL_ACT_FP32 && storage != ISL_ACT_FP16) return fail(ISL_E_ARG, "unknown activation storage");
  // (arenas are kept per storage and captured graphs keyed by it: a switch re-plans the next run)
  net->act_storage = storage;
  return ISL_OK;
}

int isl_net_get_act_storage(const isl_net* net) { return net ? net->act_storage : fail(ISL_E_ARG, "net is NULL"); }

int isl_net_act_storage_active(const isl_net* net) {
  return net ? (net->a16_active ? 1 : 0) : fail(ISL_E_ARG, "net is NULL");
}

int isl_lane_stream_create(int device, int priority_class, void** stream) {
  if (!stream) return fail(ISL_E_ARG, "stream is NULL");
  if (priority_class < -1 || priority_class > 1) return fail(ISL_E_ARG, "priority class must be -1, 0 or 1");
  *stream = nullptr;
  int cur = 0;
  HIP_OK(hipGetDevice(&cur));
  if (device != cur) HIP_OK(hipSetDevice(device));
  int least = 0, greatest = 0;
  hipError_t c = hipDeviceGetStreamPriorityRange(&least, &greatest);
  hipStream_t s = nullptr;
  if (c == hipSuccess) {
    // lower numbers are greater priorities: greatest <= mid <= least
    const int prio = priority_class < 0 ? greatest : priority_class > 0 ? least : greatest + (least - greatest + 1) / 2;
    c = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio);
  }
  if (device != cur) (void)hipSetDevice(cur);
  if (c != hipSuccess) return fail(ISL_E_HIP, std::string("hipStreamCreateWithPriority: ") + hipGetErrorString(c));
  *stream = (void*)s;
  return ISL_OK;
}

int isl_lane_stream_destroy(void* stream) {
  if (!stream) return ISL_OK;
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  HIP_OK(hipStreamDestroy((hipStream_t)stream));
  return ISL_OK;
}

int isl_net_set_graph(isl_net* net, int on) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (on < 0 || on > 1) return fail(ISL_E_ARG, "graph mode must be 0 or 1");
  net->graph = on;
  return ISL_OK;
}

int isl_net_set_split_k(isl_net* net, int mode) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (mode < 0 || mode > 2) return fail(ISL_E_ARG, "split-K mode must be 0, 1 or 2");
  net->split_k = mode;
  return ISL_OK;
}

int isl_net_check(isl_net* net, int clear) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (!net->d_flag) return ISL_OK;
  HIP_OK(hipSetDevice(net->device));
  int f = 0;
  // the convs ran on the callers' streams, which may be non-blocking (torch's): a null-stream
  // copy alone would not wait for them, so wait for the events recorded behind them (not the
  // whole device: other streams' work goes on)
  {
    const int rc = wait_flag_streams(net);
    if (rc) return rc;
  }
  HIP_OK(hipMemcpy(&f, net->d_flag, sizeof(int), hipMemcpyDeviceToHost));
  if (f && clear) {
    const int zero = 0;   // a blocking copy: cleared before the next run on any stream
    HIP_OK(hipMemcpy(net->d_flag, &zero, sizeof(int), hipMemcpyHostToDevice));
    ++net->range_trips_host;   // one trip per cleared flag (a check without clear counts nothing)
  }
  if (f) return fail(ISL_E_RANGE, "an activation left the split-fp16 range (|x| >= 65504); re-run with ISL_ALGO_DIRECT");
  return ISL_OK;
}

int isl_net_check_async(isl_net* net, int32_t* h_flag, void* stream) {
  if (!net || !h_flag) return fail(ISL_E_ARG, "NULL argument");
  if (!net->d_flag) { *h_flag = 0; return ISL_OK; }
  HIP_OK(hipSetDevice(net->device));
  hipStream_t s = (hipStream_t)stream;
  if (net->d_trips) HIP_OK(launch_range_count(net->d_flag, net->d_trips, s));
  HIP_OK(hipMemcpyAsync(h_flag, net->d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemsetAsync(net->d_flag, 0, sizeof(int), s));
  return note_flag_stream(net, s);
}

int isl_net_range_info(isl_net* net, int64_t* trips) {
  if (!net || !trips) return fail(ISL_E_ARG, "NULL argument");
  unsigned long long d = 0;
  if (net->d_trips) {
    HIP_OK(hipSetDevice(net->device));
    // range_count_kernel runs on the caller's (non-blocking) stream, which a null-stream copy
    // does not wait for: wait for the events recorded behind it
    const int rc = wait_flag_streams(net);
    if (rc) return rc;
    HIP_OK(hipMemcpy(&d, net->d_trips, sizeof(d), hipMemcpyDeviceToHost));
  }
  *trips = (int64_t)(net->range_trips_host + (long long)d);
  return ISL_OK;
}

const int* isl_net_range_flag(const isl_net* net) { return net ? net->d_flag : nullptr; }

int isl_net_arena_info(const isl_net* net, int64_t* bytes, int* n_arenas) {
  if (!net) return fail(ISL_E_ARG, "net is NULL");
  if (bytes) *bytes = (int64_t)net->plans_bytes;
  if (n_arenas) *n_arenas = (int)net->plans.size();
  return ISL_OK;
}

int isl_net_run(isl_net* net, float* d_out0, float* d_out1, void* stream) {
  if (!net || !net->arena) return fail(ISL_E_STATE, "isl_net_run before isl_net_preprocess");
  int rc = prepare(net);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // The input sits in the arena isl_net_preprocess* planned.  If the algorithm, precision or
  // storage changed since (e.g. an ISL_ALGO_DIRECT recompute without a new preprocess), this run
  // may need the size's other arena: plan it and carry the fp32 net input over, in stream order.
  if (act16_for(net, net->pn, net->ph, net->pw) != net->cur->a16) {
    const void* old_base = net->arena;
    const Act old_in = net->act[net->in_buf];
    if ((rc = plan(net, net->pn, net->ph, net->pw, s))) return rc;
    bool alive = false;
    for (auto& kv : net->plans) alive |= kv.second.base == old_base;
    if (!alive) return fail(ISL_E_STATE, "isl_net_run: the arena holding the input was evicted; preprocess again");
    HIP_OK(hipMemcpyAsync(net->act[net->in_buf].base, old_in.base, old_in.bytes(), hipMemcpyDeviceToDevice, s));
  }
  if ((rc = run_ops(net, s))) return rc;
  return copy_outputs(net, d_out0, d_out1, s);
}

// ---- isl_debug_conv: one layer on host arrays, with an output canary and an input poison ----

namespace {

constexpr uint32_t DBG_CANARY32 = 0x7fc5a5a5u;   // quiet NaNs with payloads: no layer produces them
constexpr uint16_t DBG_CANARY16 = 0x7e5au;
constexpr uint32_t DBG_POISON32 = 0x7fd1d1d1u;
constexpr uint16_t DBG_POISON16 = 0x7f1du;

// Host image of an activation buffer (isl::Act layout) of 4- or 2-byte elements with a chunk
// plane and 1024 pixels of slack on either side.
struct DbgBuf {
  Act a;
  size_t slack = 0;
  std::vector<uint8_t> h;
  void* d = nullptr;
  size_t elems() const { return 2 * slack + a.frame_elems() * a.n; }
  size_t bytes() const { return elems() * a.esize; }
  void init(int n, int H, int W, int pad, int cs, int esize) {
    a.n = n; a.H = H; a.W = W; a.pad = pad; a.cs = cs; a.esize = esize;
    slack = a.chunk_elems() + 8192;   // more than the longest staged run of any tile (576 pixels)
  }
  void alloc() { h.assign(bytes(), 0); }   // (after the caller's size check)
  void fill(size_t i0, size_t cnt, uint32_t b32, uint16_t b16) {
    if (a.esize == 4) { uint32_t* p = (uint32_t*)h.data(); std::fill(p + i0, p + i0 + cnt, b32); }
    else { uint16_t* p = (uint16_t*)h.data(); std::fill(p + i0, p + i0 + cnt, b16); }
  }
  size_t chunk_at(int f, int chunk) const { return slack + ((size_t)f * (a.cs / 8) + chunk) * a.chunk_elems(); }
  size_t at(int f, int ch, int y, int x) const {
    return chunk_at(f, ch / 8) + ((size_t)(y + a.pad) * (a.W + 2 * a.pad) + x + a.pad) * 8 + ch % 8;
  }
  void put(size_t i, float v) {
    if (a.esize == 4) ((float*)h.data())[i] = v;
    else ((_Float16*)h.data())[i] = (_Float16)v;   // round to nearest even
  }
  float get(size_t i) const { return a.esize == 4 ? ((const float*)h.data())[i] : (float)((const _Float16*)h.data())[i]; }
  uint32_t bits(size_t i) const { return a.esize == 4 ? ((const uint32_t*)h.data())[i] : ((const uint16_t*)h.data())[i]; }
  void* dev() const { return (uint8_t*)d + slack * a.esize; }   // the buffer proper
};

// Counts the elements of `b` outside (frame interior) x [c0, c1) whose bits differ from the canary
// (where zero_c0 <= channel < c1 inside the footprint: from +0 instead), and the footprint's
// elements that still hold it.
static void dbg_scan(const DbgBuf& b, int c0, int c1, int zero_c0, int stage, isl_debug_conv_result* r) {
  const uint32_t canary = b.a.esize == 4 ? DBG_CANARY32 : DBG_CANARY16;
  const size_t body = b.a.frame_elems() * b.a.n, ce = b.a.chunk_elems(), fe = b.a.frame_elems();
  const int Wp = b.a.W + 2 * b.a.pad;
  for (size_t i = 0; i < b.elems(); ++i) {
    const uint32_t v = b.bits(i);
    int f = -1, chunk = i < b.slack ? -1 : 1, y = 0, x = (int)(i < b.slack ? i : i - b.slack - body), lane = 0;
    bool inside = false, gap = false;
    if (i >= b.slack && i < b.slack + body) {
      const size_t rel = i - b.slack, rf = rel % fe, rc = rf % ce;
      f = (int)(rel / fe); chunk = (int)(rf / ce); lane = (int)(rc % 8);
      y = (int)(rc / 8 / Wp) - b.a.pad; x = (int)(rc / 8 % Wp) - b.a.pad;
      const int ch = chunk * 8 + lane;
      inside = y >= 0 && y < b.a.H && x >= 0 && x < b.a.W && ch >= c0 && ch < c1;
      gap = inside && ch >= zero_c0;
    }
    if (inside && !gap) {
      if (v == canary) ++r->unwritten;
      continue;
    }
    if (gap ? v == 0 : v == canary) continue;
    if (r->stray_writes++ == 0) {
      r->stray_stage = stage; r->stray_frame = f; r->stray_chunk = chunk; r->stray_y = y; r->stray_x = x;
      r->stray_lane = lane;
    }
  }
}

}  // namespace

int isl_debug_conv(const isl_debug_conv_desc* dp, const float* x, const float* wgt, const float* bias,
                   const float* slope, float* y, float* y_pool, isl_debug_conv_result* res) {
  if (!dp || !x || !wgt || !bias || !y || !res) return fail(ISL_E_ARG, "isl_debug_conv: NULL argument");
  const isl_debug_conv_desc d = *dp;
  *res = isl_debug_conv_result{};
  auto bad = [](const char* what) { return fail(ISL_E_ARG, std::string("isl_debug_conv: ") + what); };
  for (int v : d.reserved) if (v) return bad("reserved field not zero");
  if (d.n <= 0 || d.n > 256 || d.h <= 0 || d.w <= 0 || (long long)d.h * d.w > (1 << 20)) return bad("bad frame count or plane");
  if (d.cin <= 0 || d.cin > 1024 || d.cout <= 0 || d.cout > 1024) return bad("bad channel count");
  if (d.ks != 1 && d.ks != 3 && d.ks != 7) return bad("ks is 1, 3 or 7");
  if (d.act != ACT_NONE && d.act != ACT_RELU && d.act != ACT_PRELU) return bad("act is 0, 1 or 2");
  if (d.act == ACT_PRELU && !slope) return bad("PReLU without slopes");
  if (d.kernel < ISL_DBG_X3 || d.kernel > ISL_DBG_RGB) return bad("unknown kernel");
  const bool x3 = d.kernel == ISL_DBG_X3, rgb = d.kernel == ISL_DBG_RGB;
  if ((d.f16 | d.act16 | d.allow_split | d.hpool | d.vin) & ~1) return bad("switches are 0 or 1");
  if (d.act16 && !d.f16) return bad("act16 needs f16");
  if (d.f16 && !x3 && !rgb) return bad("f16 is a form of the x3 and rgb kernels");
  if ((d.hpool || d.vin || d.allow_split) && !x3) return bad("hpool, vin and allow_split are conv_x3's");
  if ((d.in_pad != 1 && d.in_pad != 3) || (d.out_pad != 1 && d.out_pad != 3) || d.in_pad < d.ks / 2)
    return bad("rings are 1 or 3 pixels, in_pad >= ks / 2");
  if (d.nseg < 1 || d.nseg > 4) return bad("1 to 4 input segments");
  // the channel map: the segments tile the logical channels, and do not overlap physically
  int extent = 0;
  std::vector<int> l2p(d.cin, -1);
  for (int i = 0; i < d.nseg; ++i) {
    const isl_debug_seg& sg = d.seg[i];
    if (sg.len <= 0 || sg.phys < 0 || sg.logical < 0 || sg.logical + sg.len > d.cin || sg.phys + sg.len > 1024)
      return bad("bad segment");
    for (int k = 0; k < sg.len; ++k) {
      if (l2p[sg.logical + k] >= 0) return bad("segments overlap");
      l2p[sg.logical + k] = sg.phys + k;
    }
    extent = std::max(extent, sg.phys + sg.len);
  }
  const int cin_phys = round8(extent);
  {
    std::vector<char> used(cin_phys, 0);
    for (int p : l2p) {
      if (p < 0) return bad("a logical channel without a segment");
      if (used[p]++) return bad("segments overlap");
    }
  }
  if ((d.in_cs | d.in_coff | d.out_cs | d.out_coff) & 7 || d.in_coff < 0 || d.out_coff < 0 ||
      d.in_coff + cin_phys > d.in_cs || d.out_coff + round8(d.cout) > d.out_cs || d.in_cs > 2048 || d.out_cs > 2048)
    return bad("slices: multiples of 8 inside their buffers");
  if (rgb && (d.cin != 3 || d.nseg != 1 || d.seg[0].phys != 0)) return bad("the rgb kernel takes 3 channels at the head of one chunk");
  if (d.vin && (d.in_coff || d.in_cs != cin_phys)) return bad("vin reads a whole pair-max buffer");
  if (d.hpool && (d.out_coff || (d.w & 1))) return bad("hpool writes a whole pair-max buffer of an even width");
  if (d.hpool && !y_pool) return bad("hpool without y_pool");

  ConvLayer c = mk("debug", d.cin, d.cout, d.ks, d.act);
  c.w.assign(wgt, wgt + (size_t)d.cout * d.cin * d.ks * d.ks);
  c.b.assign(bias, bias + d.cout);
  if (d.act == ACT_PRELU) c.s.assign(slope, slope + d.cout);
  for (int i = 0; i < d.nseg; ++i) c.cmap.push_back({d.seg[i].logical, d.seg[i].phys, d.seg[i].len});
  c.cin_phys = cin_phys;
  c.bco = conv_bco_for(d.cout);
  c.wbco = d.ks == 3 ? wino_bco_for(d.cout) : 0;
  if (d.kernel == ISL_DBG_WINO && !c.wbco) return bad("shape not eligible for the fp32 Winograd kernel");

  // buffers
  const int esz_in = d.act16 && !rgb ? 2 : 4, esz_out = d.act16 ? 2 : 4;
  DbgBuf in, out, pool;
  if (d.vin) in.init(d.n, 2 * d.h, d.w, 0, d.in_cs, esz_in);
  else in.init(d.n, d.h, d.w, d.in_pad, d.in_cs, esz_in);
  if (d.hpool) out.init(d.n, d.h, d.w / 2, 0, d.out_cs, esz_out);
  else out.init(d.n, d.h, d.w, d.out_pad, d.out_cs, esz_out);
  if (d.hpool) pool.init(d.n, d.h / 2, d.w / 2, d.out_pad, d.out_cs, esz_out);
  // (sizes first: the host images are allocated only once every buffer is within the limit)
  if (in.bytes() > (256u << 20) || out.bytes() > (256u << 20) || (d.hpool && pool.bytes() > (256u << 20)))
    return bad("buffer over 256 MiB");
  in.alloc();
  out.alloc();
  if (d.hpool) pool.alloc();
  in.fill(0, in.elems(), DBG_POISON32, DBG_POISON16);
  for (int f = 0; f < d.n; ++f) {
    for (int ch = 0; ch < cin_phys / 8; ++ch) in.fill(in.chunk_at(f, d.in_coff / 8 + ch), in.a.chunk_elems(), 0, 0);
    for (int lc = 0; lc < d.cin; ++lc) {
      const int pc = d.in_coff + l2p[lc];
      if (d.vin) {
        const float* xp = x + ((size_t)f * d.cin + lc) * 4 * d.h * d.w;
        for (int yy = 0; yy < 2 * d.h; ++yy)
          for (int xx = 0; xx < d.w; ++xx)
            in.put(in.at(f, pc, yy, xx), std::max(xp[(size_t)yy * 2 * d.w + 2 * xx], xp[(size_t)yy * 2 * d.w + 2 * xx + 1]));
      } else {
        const float* xp = x + ((size_t)f * d.cin + lc) * d.h * d.w;
        for (int yy = 0; yy < d.h; ++yy)
          for (int xx = 0; xx < d.w; ++xx) in.put(in.at(f, pc, yy, xx), xp[(size_t)yy * d.w + xx]);
      }
    }
  }
  out.fill(0, out.elems(), DBG_CANARY32, DBG_CANARY16);
  if (d.hpool) pool.fill(0, pool.elems(), DBG_CANARY32, DBG_CANARY16);

  const size_t nb = ((size_t)d.cout + 255) / 256 * 256 + 256;   // bias / slopes padded to any channel tile
  const std::vector<float> hb = build_param(c, PB_BIAS, nb), hs = build_param(c, PB_SLOPE, nb);

  ConvLaunch L;
  L.in_pad = d.in_pad; L.in_cs = d.in_cs; L.in_coff = d.in_coff;
  L.out_pad = d.hpool ? 0 : d.out_pad; L.out_cs = d.out_cs; L.out_coff = d.out_coff;
  L.n = d.n; L.H = d.h; L.W = d.w; L.ks = d.ks; L.cin_chunks = cin_phys / 8;
  L.cout = d.cout; L.bco = c.bco; L.act = d.act;
  L.allow_split = d.allow_split;
  L.vin = d.vin;
  // the choices plan_steps makes for a launch, in its order; the shape checks need no device memory
  const X3Switches sw = x3_switches();
  int kind = PK_DIRECT;
  if (x3) {
    if (!x3_fits(L)) return bad("shape does not fit conv_x3");
    if (d.vin && !x3_vin_ok(L, device_cus(), sw)) return bad("no pooled-input variant for this launch (x3_vin_ok)");
    ConvLaunch Lw = L;
    Lw.bco = 256;
    if (x3_wide1_layer(d.ks, d.cout, cin_phys) && x3_wide1(Lw, device_cus(), sw)) L.bco = 256;
    L.f16 = d.f16;
    if (d.act16) {
      if (!x3_act16_ok(L, device_cus(), sw)) return bad("no fp16-storage form of this launch (x3_act16_ok)");
      L.act16 = 1;
    }
    if (d.hpool) {
      if (!x3_hpool_ok(L, device_cus(), sw)) return bad("no pair-max epilogue for this launch (x3_hpool_ok)");
      L.hpool = 1;
    }
    kind = L.bco == 256 ? PK_X3_WIDE : PK_X3;
  } else if (rgb) {
    L.f16 = d.f16; L.act16 = d.act16;
    if (!rgb_layer(c) || !x3_rgb_fits(L)) return bad("shape does not fit the rgb kernel");
    kind = PK_RGB;
  } else if (d.kernel == ISL_DBG_WINO2) {
    if (d.ks != 3 || d.cout % 64 || !wino_f16_fits(L)) return bad("shape not eligible for the Winograd kernel");
    kind = PK_WINO_F16;
  } else if (d.kernel == ISL_DBG_WINO) {
    L.bco = c.wbco;
    kind = PK_WINO;
  }
  const HostPack pk = build_pack(c, kind, d.f16, &L.wscale_inv);

  std::vector<void*> owned;
  int flag = 0;
  auto dmalloc = [&](void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 16));
    if (e == hipSuccess) owned.push_back(*p);
    return e;
  };
  auto run = [&]() -> int {
    float *d_b = nullptr, *d_s = nullptr, *d_ws = nullptr;
    void* d_w = nullptr;
    int* d_flag = nullptr;
    HIP_OK(dmalloc(&in.d, in.bytes()));
    HIP_OK(dmalloc(&out.d, out.bytes()));
    HIP_OK(dmalloc((void**)&d_b, nb * 4));
    HIP_OK(dmalloc((void**)&d_s, nb * 4));
    HIP_OK(dmalloc(&d_w, pk.bytes()));
    HIP_OK(dmalloc((void**)&d_flag, 4));
    HIP_OK(hipMemcpy(in.d, in.h.data(), in.bytes(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(out.d, out.h.data(), out.bytes(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_b, hb.data(), nb * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_s, hs.data(), nb * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_w, pk.data(), pk.bytes(), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_flag, 0, 4));
    L.in = (const float*)in.dev(); L.out = (float*)out.dev();
    L.bias = d_b; L.slope = d_s; L.range_flag = d_flag;
    if (pk.f16.empty()) L.wpk = (const float*)d_w; else L.wx3 = d_w;
    if (x3) {
      const X3Choice ch = x3_choose(L, device_cus(), sw);
      const size_t need = ch.ws_floats;
      if (need > (64u << 20)) return bad("split-K workspace over 256 MiB");
      if (need) {   // partial sums: a NaN where a reduce reads what no block wrote
        std::vector<uint32_t> hw(need, DBG_POISON32);
        HIP_OK(dmalloc((void**)&d_ws, need * 4));
        HIP_OK(hipMemcpy(d_ws, hw.data(), need * 4, hipMemcpyHostToDevice));
        L.ws = d_ws; L.ws_floats = need;
      }
      HIP_OK(launch_conv_x3(L, ch, sw, 0));
      res->variant = ch.code;
    } else if (rgb) {
      HIP_OK(launch_conv_x3_rgb(L, 0));
      res->variant = x3_choose_rgb(L).code;
    } else if (d.kernel == ISL_DBG_WINO2) {
      HIP_OK(launch_wino_f16(L, 0));
      res->variant = x3_variant_code(X3V_W2, 3, 128, 64);
    } else if (d.kernel == ISL_DBG_WINO) {
      HIP_OK(launch_wino(L, 0));
    } else {
      HIP_OK(launch_conv(L, 0));
    }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.h.data(), out.d, out.bytes(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
    if (d.hpool) {
      // the arena's gap channels are zero (plan(): "zero rings and gap channels, once"); the pool
      // copies whole chunks
      std::vector<uint8_t> keep = out.h;
      for (int f = 0; f < d.n; ++f)
        for (int ch = d.cout; ch < round8(d.cout); ++ch)
          for (int yy = 0; yy < out.a.H; ++yy)
            for (int xx = 0; xx < out.a.W; ++xx) out.put(out.at(f, ch, yy, xx), 0.f);
      HIP_OK(hipMemcpy(out.d, out.h.data(), out.bytes(), hipMemcpyHostToDevice));
      out.h.swap(keep);
      HIP_OK(dmalloc(&pool.d, pool.bytes()));
      HIP_OK(hipMemcpy(pool.d, pool.h.data(), pool.bytes(), hipMemcpyHostToDevice));
      Act ha = out.a, pa = pool.a;
      ha.base = (float*)out.dev(); pa.base = (float*)pool.dev();
      HIP_OK(launch_vpool2(ha, pa, d.cout, 0));
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipMemcpy(pool.h.data(), pool.d, pool.bytes(), hipMemcpyDeviceToHost));
    }
    return ISL_OK;
  };
  const int rc = run();
  for (void* p : owned) (void)hipFree(p);
  if (rc) return rc;
  res->range_flag = flag;
  dbg_scan(out, d.out_coff, d.out_coff + d.cout, d.out_coff + d.cout, 0, res);
  if (d.hpool) dbg_scan(pool, 0, round8(d.cout), d.cout, 1, res);
  for (int f = 0; f < d.n; ++f)
    for (int co = 0; co < d.cout; ++co) {
      float* yp = y + ((size_t)f * d.cout + co) * out.a.H * out.a.W;
      for (int yy = 0; yy < out.a.H; ++yy)
        for (int xx = 0; xx < out.a.W; ++xx) yp[(size_t)yy * out.a.W + xx] = out.get(out.at(f, d.out_coff + co, yy, xx));
      if (!d.hpool) continue;
      float* pp = y_pool + ((size_t)f * d.cout + co) * pool.a.H * pool.a.W;
      for (int yy = 0; yy < pool.a.H; ++yy)
        for (int xx = 0; xx < pool.a.W; ++xx) pp[(size_t)yy * pool.a.W + xx] = pool.get(pool.at(f, co, yy, xx));
    }
  if (flag && d.range_error) return fail(ISL_E_RANGE, "isl_debug_conv: the layer left the fp16 split range");
  return ISL_OK;
}

int isl_debug_conv3x3(const float* x, int n, int cin, int h, int w, const float* wgt, const float* bias,
                      const float* slope, int cout, int kernel, float* y) {
  if (!x || !wgt || !bias || !slope || !y) return fail(ISL_E_ARG, "isl_debug_conv3x3: NULL argument");
  if (n <= 0 || n > 64 || cin <= 0 || cin > 1024 || cin % 8 || cout <= 0 || cout > 1024 || h <= 0 || w <= 0 ||
      (long long)h * w > (1 << 20) || (kernel != 0 && kernel != 1))
    return fail(ISL_E_ARG, "isl_debug_conv3x3: bad argument");
  isl_debug_conv_desc d{};
  d.n = n; d.h = h; d.w = w; d.cin = cin; d.cout = cout; d.ks = 3; d.act = ACT_PRELU;
  d.kernel = kernel == 1 ? ISL_DBG_WINO2 : ISL_DBG_X3;
  d.in_pad = d.out_pad = 1;
  d.in_cs = cin; d.out_cs = round8(cout);
  d.nseg = 1;
  d.seg[0] = {0, 0, cin};
  d.range_error = 1;
  isl_debug_conv_result r;
  return isl_debug_conv(&d, x, wgt, bias, slope, y, nullptr, &r);
}

}  // extern "C"
