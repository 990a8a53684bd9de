// bvh_opt.cpp — reinsertion-optimised topology for the compact traversal nodes (host, C++). See bvh_opt.h.
#include "bvh_opt.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>

#include "bvh.h"

namespace ptgs {

namespace {

constexpr float kFar = 1e29f;  // (bvh.cpp quantize_bvh4: the empty slots' 1e30 planes and anything as far)

struct Node2 {
  float lo[3], hi[3];
  int32_t parent = -1;
  int32_t c[2] = {-1, -1};  // interior: the two children
  int32_t link = 0;         // leaf: the canonical link (< 0)
  bool leaf() const { return link < 0; }
};

double half_area(const float* lo, const float* hi) {
  const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
  if (dx < 0 || dy < 0 || dz < 0) return 0.0;
  return dx * dy + dy * dz + dz * dx;
}
double union_area(const Node2& a, const Node2& b) {
  float lo[3], hi[3];
  for (int k = 0; k < 3; ++k) { lo[k] = std::min(a.lo[k], b.lo[k]); hi[k] = std::max(a.hi[k], b.hi[k]); }
  return half_area(lo, hi);
}
bool real_box(const float* f, int j) {
  for (int a = 0; a < 3; ++a) {
    const float lo = f[(2 * a) * 4 + j], hi = f[(2 * a + 1) * 4 + j];
    if (!(std::fabs(lo) < kFar && std::fabs(hi) < kFar && lo <= hi)) return false;
  }
  return true;
}

struct Tree2 {
  std::vector<Node2> n;
  std::vector<double> area;
  int32_t root = -1;

  int32_t add(const Node2& x) {
    n.push_back(x);
    area.push_back(half_area(x.lo, x.hi));
    return (int32_t)n.size() - 1;
  }
  int32_t join(int32_t a, int32_t b) {
    Node2 x;
    for (int k = 0; k < 3; ++k) { x.lo[k] = std::min(n[a].lo[k], n[b].lo[k]); x.hi[k] = std::max(n[a].hi[k], n[b].hi[k]); }
    x.c[0] = a; x.c[1] = b;
    const int32_t i = add(x);
    n[a].parent = i; n[b].parent = i;
    return i;
  }
  // the boxes of x and its ancestors from their children; stops at the first box that does not move
  void refit(int32_t x) {
    for (; x >= 0; x = n[x].parent) {
      Node2& p = n[x];
      const Node2 &a = n[p.c[0]], &b = n[p.c[1]];
      bool same = true;
      for (int k = 0; k < 3; ++k) {
        const float lo = std::min(a.lo[k], b.lo[k]), hi = std::max(a.hi[k], b.hi[k]);
        same = same && lo == p.lo[k] && hi == p.hi[k];
        p.lo[k] = lo; p.hi[k] = hi;
      }
      if (same) return;
      area[x] = half_area(p.lo, p.hi);
    }
  }
  void replace_child(int32_t parent, int32_t was, int32_t now) {
    if (parent < 0) root = now;
    else n[parent].c[n[parent].c[0] == was ? 0 : 1] = now;
    n[now].parent = parent;
  }
};

// the BVH2 of the canonical 4-wide tree: false for a tree this optimiser leaves alone
struct Binarise {
  const float* n4;
  uint32_t num;
  Tree2& t;
  std::vector<uint8_t> seen;
  bool ok = true;

  int32_t node(uint32_t i, uint32_t depth) {
    if (i >= num || seen[i] || depth > 4096) { ok = false; return -1; }
    seen[i] = 1;
    const float* f = n4 + 32 * (size_t)i;
    int32_t e[4];
    int cnt = 0;
    for (int j = 0; j < 4 && ok; ++j) {
      int32_t link;
      std::memcpy(&link, &f[24 + j], 4);
      if (link == 0) continue;  // an empty slot (the root is no child)
      if (link < 0) {
        if (!real_box(f, j)) { ok = false; break; }
        Node2 x;
        for (int a = 0; a < 3; ++a) { x.lo[a] = f[(2 * a) * 4 + j]; x.hi[a] = f[(2 * a + 1) * 4 + j]; }
        x.link = link;
        e[cnt++] = t.add(x);
      } else {
        e[cnt++] = node((uint32_t)link, depth + 1);
      }
    }
    if (!ok || cnt < 2) { ok = false; return -1; }
    while (cnt > 1) {  // pair the two entries of smallest union area (ties: the first pair)
      int ba = 0, bb = 1;
      double best = std::numeric_limits<double>::infinity();
      for (int a = 0; a < cnt; ++a)
        for (int b = a + 1; b < cnt; ++b) {
          const double u = union_area(t.n[e[a]], t.n[e[b]]);
          if (u < best) { best = u; ba = a; bb = b; }
        }
      e[ba] = t.join(e[ba], e[bb]);
      for (int k = bb; k + 1 < cnt; ++k) e[k] = e[k + 1];
      --cnt;
    }
    return e[0];
  }
};

typedef std::pair<double, int32_t> Cand;  // (induced cost, node): a min-heap by std::greater

void reinsertion_pass(Tree2& t, std::vector<Cand>& heap) {
  std::vector<int32_t> order;
  order.reserve(t.n.size());
  for (int32_t i = 0; i < (int32_t)t.n.size(); ++i)
    if (i != t.root) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return t.area[a] != t.area[b] ? t.area[a] > t.area[b] : a < b;
  });
  for (const int32_t x : order) {
    const int32_t p = t.n[x].parent;
    if (x == t.root || p == t.root) continue;
    const int32_t g = t.n[p].parent;
    const int32_t s = t.n[p].c[t.n[p].c[0] == x ? 1 : 0];
    // detach: the sibling takes the parent's place
    t.replace_child(g, p, s);
    t.refit(g);
    const double ax = t.area[x];
    // the place it came from is the bound to beat: a tree whose costs all tie keeps its shape
    double best = union_area(t.n[s], t.n[x]);
    for (int32_t a = g; a >= 0; a = t.n[a].parent) best += union_area(t.n[a], t.n[x]) - t.area[a];
    int32_t at = s;
    heap.clear();
    heap.push_back(Cand(0.0, t.root));
    while (!heap.empty()) {
      std::pop_heap(heap.begin(), heap.end(), std::greater<Cand>());
      const Cand c = heap.back();
      heap.pop_back();
      if (c.first + ax >= best) break;
      const Node2& y = t.n[c.second];
      const double cost = c.first + union_area(y, t.n[x]);
      if (cost < best) { best = cost; at = c.second; }
      const double below = cost - t.area[c.second];
      if (!y.leaf() && below + ax < best)
        for (int k = 0; k < 2; ++k) {
          heap.push_back(Cand(below, y.c[k]));
          std::push_heap(heap.begin(), heap.end(), std::greater<Cand>());
        }
    }
    // re-attach with the freed parent: p takes at's place and holds (at, x)
    t.replace_child(t.n[at].parent, at, p);
    t.n[p].c[0] = at; t.n[p].c[1] = x;
    t.n[at].parent = p; t.n[x].parent = p;
    for (int k = 0; k < 3; ++k) { t.n[p].lo[k] = 1.0f; t.n[p].hi[k] = 0.0f; }  // (stale: refit must not stop here)
    t.refit(p);
  }
}

// the BVH2 breadth first in build_bvh's layout (bvh.h), boxes as they are (the leaves' are already padded)
void emit_bvh2(const Tree2& t, std::vector<float>& n2) {
  std::vector<int32_t> queue;
  queue.push_back(t.root);
  std::vector<int32_t> index(t.n.size(), -1);
  index[t.root] = 0;
  for (size_t q = 0; q < queue.size(); ++q)
    for (int k = 0; k < 2; ++k) {
      const int32_t c = t.n[queue[q]].c[k];
      if (t.n[c].leaf()) continue;
      index[c] = (int32_t)queue.size();
      queue.push_back(c);
    }
  n2.assign(queue.size() * 16, 0.0f);
  for (size_t q = 0; q < queue.size(); ++q) {
    float* f = &n2[16 * q];
    const Node2& p = t.n[queue[q]];
    for (int k = 0; k < 2; ++k) {
      const Node2& c = t.n[p.c[k]];
      f[4 * k + 0] = c.lo[0]; f[4 * k + 1] = c.hi[0]; f[4 * k + 2] = c.lo[1]; f[4 * k + 3] = c.hi[1];
      f[8 + 2 * k] = c.lo[2]; f[9 + 2 * k] = c.hi[2];
      const int32_t link = c.leaf() ? c.link : index[p.c[k]];
      std::memcpy(&f[12 + k], &link, 4);
    }
  }
}

// collapse_bvh4's entry and its float area (bvh.cpp), restated: the budgeted collapse orders by the same numbers
struct Ent4 {
  float lo[3], hi[3];
  int32_t ref;
};
void bvh2_children(const float* n, Ent4 e[2]) {
  int32_t c0, c1;
  std::memcpy(&c0, &n[12], 4);
  std::memcpy(&c1, &n[13], 4);
  e[0] = Ent4{{n[0], n[2], n[8]}, {n[1], n[3], n[9]}, c0};
  e[1] = Ent4{{n[4], n[6], n[10]}, {n[5], n[7], n[11]}, c1};
}
float ent_area(const Ent4& e) {
  float d[3];
  for (int a = 0; a < 3; ++a) d[a] = std::max(0.0f, e.hi[a] - e.lo[a]);
  return d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
}

// interior height of every BVH2 node (a node of two leaves: 1), children after parents (emit_bvh2, build_bvh)
void bvh2_heights(const std::vector<float>& n2, std::vector<uint32_t>& h) {
  const size_t num = n2.size() / 16;
  h.assign(num, 0u);
  for (size_t i = num; i-- > 0;) {
    uint32_t m = 0;
    for (int k = 0; k < 2; ++k) {
      int32_t c;
      std::memcpy(&c, &n2[16 * i + 12 + k], 4);
      if (c >= 0) m = std::max(m, h[(size_t)c]);
    }
    h[i] = 1u + m;
  }
}

}  // namespace

uint32_t bvh2_height(const std::vector<float>& n2) {
  std::vector<uint32_t> h;
  bvh2_heights(n2, h);
  return h.empty() ? 0u : h[0];
}

bool collapse_bvh4_budget(const std::vector<float>& n2, std::vector<float>& n4, uint32_t& num4, uint32_t& max_stack,
                          uint32_t& depth4, int max_children, uint32_t need_limit) {
  n4.clear();
  num4 = 0; max_stack = 0; depth4 = 0;
  std::vector<uint32_t> h2;
  bvh2_heights(n2, h2);
  if (h2.empty() || need_limit == 0 || h2[0] >= need_limit) return false;
  max_children = std::max(2, std::min(4, max_children));
  auto height = [&](const Ent4& e) { return e.ref >= 0 ? h2[(size_t)e.ref] : 0u; };
  struct Item { int32_t b2; uint32_t slot, budget; };
  std::vector<Item> queue;  // breadth first, as collapse_bvh4: the same slots when no budget binds
  std::vector<std::vector<uint32_t>> kids;
  std::vector<uint32_t> ncount;
  queue.push_back(Item{0, 0u, need_limit - 1u});
  n4.assign(32, 0.0f);
  kids.emplace_back();
  ncount.push_back(0);
  for (size_t q = 0; q < queue.size(); ++q) {
    const Item it = queue[q];  // (budget >= the node's height >= 1: its two children fit budget - 1)
    Ent4 list[4];
    int cnt = 2;
    bvh2_children(&n2[16 * (size_t)it.b2], list);
    while (cnt < max_children) {
      // interior children by descending area (ties: the first, collapse_bvh4's choice); the first whose opening
      // leaves every child a height within budget - cnt (cnt + 1 children: cnt entries pushed above them)
      int order[4], no = 0;
      for (int k = 0; k < cnt; ++k)
        if (list[k].ref >= 0) order[no++] = k;
      std::stable_sort(order, order + no, [&](int a, int b) { return ent_area(list[a]) > ent_area(list[b]); });
      int best = -1;
      Ent4 sub[2];
      for (int o = 0; o < no && best < 0; ++o) {
        if (it.budget < (uint32_t)cnt) break;
        const uint32_t room = it.budget - (uint32_t)cnt;
        bvh2_children(&n2[16 * (size_t)list[order[o]].ref], sub);
        bool fits = height(sub[0]) <= room && height(sub[1]) <= room;
        for (int k = 0; k < cnt && fits; ++k)
          if (k != order[o]) fits = height(list[k]) <= room;
        if (fits) best = order[o];
      }
      if (best < 0) break;
      list[best] = sub[0];
      list[cnt++] = sub[1];
    }
    float* f = &n4[32 * (size_t)it.slot];
    for (int j = 0; j < 4; ++j) {
      int32_t child = 0;
      if (j < cnt) {
        for (int a = 0; a < 3; ++a) {
          f[(2 * a) * 4 + j] = list[j].lo[a];
          f[(2 * a + 1) * 4 + j] = list[j].hi[a];
        }
        if (list[j].ref >= 0) {
          const uint32_t ni = (uint32_t)(n4.size() / 32);
          n4.resize(n4.size() + 32, 0.0f);
          f = &n4[32 * (size_t)it.slot];  // (resize may move the storage)
          queue.push_back(Item{list[j].ref, ni, it.budget - (uint32_t)(cnt - 1)});
          kids.emplace_back();
          ncount.push_back(0);
          kids[it.slot].push_back(ni);
          child = (int32_t)ni;
        } else {
          child = list[j].ref;
        }
      } else {
        for (int a = 0; a < 6; ++a) f[a * 4 + j] = 1e30f;  // empty: a point box no ray reaches
      }
      std::memcpy(&f[24 + j], &child, 4);
    }
    ncount[it.slot] = (uint32_t)cnt;
  }
  num4 = (uint32_t)(n4.size() / 32);
  std::vector<uint32_t> need(num4, 0), dep(num4, 1);
  for (size_t i = num4; i-- > 0;) {
    uint32_t m = 0, d = 0;
    for (uint32_t k : kids[i]) { m = std::max(m, need[k]); d = std::max(d, dep[k]); }
    need[i] = (ncount[i] - 1) + m;
    dep[i] = 1 + d;
  }
  max_stack = need[0];
  depth4 = dep[0];
  return max_stack < need_limit;
}

double bvh4_area_sum(const float* n4, uint32_t num) {
  double sum = 0.0, root = 0.0;
  for (uint32_t i = 0; i < num; ++i) {
    const float* f = n4 + 32 * (size_t)i;
    float lo[3] = {1.0f, 1.0f, 1.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
    for (int j = 0; j < 4; ++j) {
      int32_t link;
      std::memcpy(&link, &f[24 + j], 4);
      if (link == 0 || !real_box(f, j)) continue;
      for (int a = 0; a < 3; ++a) {
        const float l = f[(2 * a) * 4 + j], h = f[(2 * a + 1) * 4 + j];
        lo[a] = any ? std::min(lo[a], l) : l;
        hi[a] = any ? std::max(hi[a], h) : h;
      }
      any = true;
    }
    const double a = any ? half_area(lo, hi) : 0.0;
    if (i == 0) root = a;
    sum += a;
  }
  return root > 0.0 ? sum / root : 0.0;
}

bool optimize_bvh4(const float* n4, uint32_t num, int fan, uint32_t need_limit, std::vector<float>& out,
                   TreeOptInfo& info, int passes) {
  return optimize_bvh4(n4, num, fan, &need_limit, 1, out, info, passes);
}

bool optimize_bvh4(const float* n4, uint32_t num, int fan, const uint32_t* limits, int num_limits,
                   std::vector<float>& out, TreeOptInfo& info, int passes) {
  const auto t0 = std::chrono::steady_clock::now();
  info = TreeOptInfo{};
  out.clear();
  info.area_before = bvh4_area_sum(n4, num);
  auto done = [&](bool applied) {
    info.applied = applied ? 1u : 0u;
    if (!applied) out.clear();
    info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return applied;
  };
  if (num == 0) return done(false);
  Tree2 t;
  t.n.reserve((size_t)num * 8);
  t.area.reserve((size_t)num * 8);
  Binarise b{n4, num, t, std::vector<uint8_t>(num, 0)};
  t.root = b.node(0, 0);
  if (!b.ok) return done(false);
  std::vector<Cand> heap;
  for (int p = 0; p < passes; ++p) reinsertion_pass(t, heap);
  info.passes = (uint32_t)std::max(0, passes);
  std::vector<float> n2;
  emit_bvh2(t, n2);
  info.height2 = bvh2_height(n2);
  const int fan0 = std::max(2, std::min(4, fan));
  for (int l = 0; l < num_limits; ++l) {
    const uint32_t need_limit = limits[l];
    for (int f = fan0; f >= 2; --f) {
      uint32_t num4 = 0, need = 0, depth4 = 0;
      collapse_bvh4(n2, out, num4, need, depth4, f);
      // the greedy collapse's need does not fit: at the canonical fan-out, the collapse that narrows only the
      // paths that set it (false when the BVH2's height reaches the limit: the lower fan-outs, as before)
      if (need >= need_limit && !(f == fan0 && collapse_bvh4_budget(n2, out, num4, need, depth4, f, need_limit)))
        continue;
      info.num_nodes = num4;
      info.need = need;
      info.depth = depth4;
      info.fan = (uint32_t)f;
      info.limit = need_limit;
      info.area_after = bvh4_area_sum(out.data(), num4);
      return done(true);
    }
  }
  return done(false);
}

bool make_opt_traversal_nodes(const float* n4, uint32_t num, int fan, uint32_t need_limit, bool optimise,
                              int force_key_bits, std::vector<uint32_t>& n64, StackLayout& layout, TreeOptInfo& info,
                              std::vector<float>* walked) {
  return make_opt_traversal_nodes(n4, num, fan, &need_limit, 1, optimise, force_key_bits, n64, layout, info, walked);
}

bool make_opt_traversal_nodes(const float* n4, uint32_t num, int fan, const uint32_t* limits, int num_limits,
                              bool optimise, int force_key_bits, std::vector<uint32_t>& n64, StackLayout& layout,
                              TreeOptInfo& info, std::vector<float>* walked) {
  info = TreeOptInfo{};
  std::vector<float> opt;
  if (optimise && optimize_bvh4(n4, num, fan, limits, num_limits, opt, info)) {
    if (make_traversal_nodes(opt.data(), info.num_nodes, force_key_bits, n64, layout)) {
      if (walked) walked->swap(opt);
      return true;
    }
    info.applied = 0;
  }
  if (!optimise) info.area_before = bvh4_area_sum(n4, num);  // (the report's canonical figure, either way)
  if (walked) walked->assign(n4, n4 + (size_t)num * 32);
  return make_traversal_nodes(n4, num, force_key_bits, n64, layout);
}

}  // namespace ptgs
