// bvh_opt.h — reinsertion-optimised topology for the megakernel's compact traversal nodes.
//
// The megakernel walks a copy (bvh.h make_traversal_nodes) of the final canonical 4-wide nodes. Hits do not
// depend on the tree (closest hit: a minimum over (t, gid); any-hit: an OR; the alpha hash is per gid), so that
// copy's topology is free. optimize_bvh4 rebuilds it for fewer node steps per ray:
//   binarise   each 4-wide node becomes a BVH2 of its children, pairing the two entries of smallest union area.
//              Leaves are units: their links (first triangle, count) are never split, merged or renumbered, so
//              the triangle records stay as they are. A leaf's box is its stored, padded child planes; an
//              interior box is the union of its leaves' boxes: every box stays conservative, and a subtree's
//              box still holds every candidate's entry distance (the cull at pop, pt_device.h trace_closest).
//   reinsert   kTreeOptPasses passes. A pass takes every BVH2 node but the root and its children, in descending
//              box area (ties: node index), detaches it (its sibling takes the parent's place), finds the
//              cheapest place to put it back by a branch-and-bound search from the root on the induced cost
//              (sum over ancestors a of area(a + n) - area(a)), and re-attaches it there with the freed parent.
//              Areas are summed in double. (Bittner, Hapala, Havran: Fast insertion-based optimization of
//              bounding volume hierarchies, CGF 2013.)
//   emit       the BVH2 breadth first, collapsed by collapse_bvh4 at the canonical tree's fan-out. When the
//              collapsed tree's stack need reaches need_limit: collapse_bvh4_budget at that fan-out, which
//              narrows only the paths that set the need; when the BVH2 is too high for that, the fan-outs below.
// The result is a pure function of the input bytes.
#pragma once

#include <stdint.h>
#include <vector>

#include "bvh.h"

namespace ptgs {

constexpr int kTreeOptPasses = 2;

struct TreeOptInfo {
  uint32_t applied = 0;    // 1: `out` holds the optimised nodes
  uint32_t num_nodes = 0;  // optimised 4-wide nodes, their stack need (collapse_bvh4's max_stack) and depth
  uint32_t need = 0;
  uint32_t depth = 0;
  uint32_t fan = 0;        // the fan-out the optimised tree was collapsed at
  uint32_t passes = 0;
  uint32_t limit = 0;      // the need limit the optimised tree was held to (the first of the limits it met)
  uint32_t height2 = 0;    // bvh2_height of the reinserted BVH2 (filled once it exists, applied or not)
  double area_before = 0.0;  // sum of the 4-wide nodes' box areas / the root's, canonical and optimised
  double area_after = 0.0;
  double ms = 0.0;
};

// sum over the 4-wide nodes of the area of the union of their children's boxes, over the root's (0 for a tree
// with no finite box)
double bvh4_area_sum(const float* nodes4, uint32_t num_nodes);

// Interior height of a BVH2 (bvh.h layout, children after parents): a node of two leaves has 1. It is the need
// of the BVH2's own chain at fan-out 2, and opening children never lowers it: no collapse needs less.
uint32_t bvh2_height(const std::vector<float>& nodes2);

// collapse_bvh4 (bvh.h) under a stack budget: need < need_limit. Top-down, every 4-wide node is given the
// entries it may still use: the root need_limit - 1, a child of a node with k children the node's budget less
// k - 1. A node opens its largest-area interior child, as collapse_bvh4 does, only if every child it then has is
// no higher (bvh2_height of its subtree) than the budget less the new k - 1; otherwise the next largest; it stops
// when none can open. Where the budget never binds the output is collapse_bvh4's, byte for byte. False (nodes4
// empty) when bvh2_height(nodes2) >= need_limit: no collapse fits.
bool collapse_bvh4_budget(const std::vector<float>& nodes2, std::vector<float>& nodes4, uint32_t& num_nodes4,
                          uint32_t& max_stack, uint32_t& depth4, int max_children, uint32_t need_limit);

// nodes4: the canonical 4-wide nodes (bvh.h, 128 B each) collapsed at fan-out `fan`. need_limit: the optimised
// tree's stack need stays below it. False ("not applied": `out` is empty and the caller converts the canonical
// nodes) for a tree with a box no ray can reach (the empty tree), with a link out of range, or when no fan-out
// keeps the need below the limit; info's area_before and ms are filled either way.
bool optimize_bvh4(const float* nodes4, uint32_t num_nodes, int fan, uint32_t need_limit, std::vector<float>& out,
                   TreeOptInfo& info, int passes = kTreeOptPasses);
// The same with several limits in order of preference (the megakernel's LDS depth, then LDS + overflow): one
// reinsertion, then the collapses above under the first limit, and under the next only if that one is not met.
bool optimize_bvh4(const float* nodes4, uint32_t num_nodes, int fan, const uint32_t* limits, int num_limits,
                   std::vector<float>& out, TreeOptInfo& info, int passes = kTreeOptPasses);

// What the scene upload gives the megakernel: with `optimise`, optimize_bvh4 and make_traversal_nodes (bvh.h) of
// its output; otherwise, or when the optimiser does not apply (or its output is refused by the quantiser), the
// plain conversion of the canonical nodes. `walked` (optional) gets the 4-wide nodes that were converted. False
// when the conversion of the canonical nodes is refused.
bool make_opt_traversal_nodes(const float* nodes4, uint32_t num_nodes, int fan, uint32_t need_limit, bool optimise,
                              int force_key_bits, std::vector<uint32_t>& nodes64, StackLayout& layout, TreeOptInfo& info,
                              std::vector<float>* walked = nullptr);
bool make_opt_traversal_nodes(const float* nodes4, uint32_t num_nodes, int fan, const uint32_t* limits, int num_limits,
                              bool optimise, int force_key_bits, std::vector<uint32_t>& nodes64, StackLayout& layout,
                              TreeOptInfo& info, std::vector<float>* walked = nullptr);

}  // namespace ptgs
