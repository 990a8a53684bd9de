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
//   emit       the BVH2 breadth first, collapsed by collapse_bvh4 at the canonical tree's fan-out; when the
//              collapsed tree's stack need reaches need_limit, at the fan-outs below it.
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
  double area_before = 0.0;  // sum of the 4-wide nodes' box areas / the root's, canonical and optimised
  double area_after = 0.0;
  double ms = 0.0;
};

// sum over the 4-wide nodes of the area of the union of their children's boxes, over the root's (0 for a tree
// with no finite box)
double bvh4_area_sum(const float* nodes4, uint32_t num_nodes);

// nodes4: the canonical 4-wide nodes (bvh.h, 128 B each) collapsed at fan-out `fan`. need_limit: the optimised
// tree's stack need stays below it. False ("not applied": `out` is empty and the caller converts the canonical
// nodes) for a tree with a box no ray can reach (the empty tree), with a link out of range, or when no fan-out
// keeps the need below the limit; info's area_before and ms are filled either way.
bool optimize_bvh4(const float* nodes4, uint32_t num_nodes, int fan, uint32_t need_limit, std::vector<float>& out,
                   TreeOptInfo& info, int passes = kTreeOptPasses);

// What the scene upload gives the megakernel: with `optimise`, optimize_bvh4 and make_traversal_nodes (bvh.h) of
// its output; otherwise, or when the optimiser does not apply (or its output is refused by the quantiser), the
// plain conversion of the canonical nodes. `walked` (optional) gets the 4-wide nodes that were converted. False
// when the conversion of the canonical nodes is refused.
bool make_opt_traversal_nodes(const float* nodes4, uint32_t num_nodes, int fan, uint32_t need_limit, bool optimise,
                              int force_key_bits, std::vector<uint32_t>& nodes64, StackLayout& layout, TreeOptInfo& info,
                              std::vector<float>* walked = nullptr);

}  // namespace ptgs
