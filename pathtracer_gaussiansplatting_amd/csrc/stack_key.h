// stack_key.h — the packed traversal-stack word of the path-tracer megakernel (pt_device.h trace_closest),
// shared by the kernel, the scene upload (bvh.cpp stack_layout / pack_links64) and the host check
// (tests/native/stack_cull_check.cpp).
//
//   bit 31            leaf flag (as the canonical link's sign)
//   bits 30 .. 31-W   distance key: the top W bits of the IEEE-754 pattern of the child's slab entry tn below
//                     the sign (W <= 8: exponent bits only; W = 11: the exponent and 3 mantissa bits)
//   low bits          interior node index, or for a leaf first_triangle | (count - 1) << leaf_shift
//
// tn is never negative and never NaN (it is an fmaxf against the ray's tmin), so its pattern is monotone in
// its value and clearing low bits of it is a floor: decode(encode(x)) <= x for every x >= 0, +inf included.
// The key needs no rebasing, clamp or shift: encode is one AND-OR onto the link, decode one AND. W = 0
// (key_mask 0) decodes every entry to 0.0, a bound that never culls.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTGS_SK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PTGS_SK_HD inline
#endif

namespace ptgs {

struct StackLayout {
  uint32_t key_mask;         // the key's bits in a stack word (0: no key)
  uint32_t leaf_shift;       // a packed leaf's count - 1 sits above its first triangle
  uint32_t leaf_start_mask;  // (1 << leaf_shift) - 1
  uint32_t key_bits;         // W
  uint32_t ref_bits;         // flag + payload: what the tree's links need
};

// the key's mask for W = w bits (0 .. 31)
PTGS_SK_HD uint32_t stack_key_mask(uint32_t w) { return w >= 31u ? 0x7fffffffu : (((1u << w) - 1u) << (31u - w)); }

PTGS_SK_HD uint32_t stack_f2u(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
PTGS_SK_HD float stack_u2f(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// link: a packed link (key bits clear); tn >= 0
PTGS_SK_HD uint32_t stack_pack(uint32_t link, float tn, uint32_t key_mask) { return (stack_f2u(tn) & key_mask) | link; }
// the entry's lower bound on tn
PTGS_SK_HD float stack_bound(uint32_t word, uint32_t key_mask) { return stack_u2f(word & key_mask); }
PTGS_SK_HD uint32_t stack_link(uint32_t word, uint32_t key_mask) { return word & ~key_mask; }

// canonical link (bvh.h: >= 0 interior index, < 0 leaf = ~((count - 1) << 27 | first)) <-> packed link
PTGS_SK_HD uint32_t stack_link_pack(int32_t link, const StackLayout& l) {
  if (link >= 0) return (uint32_t)link;
  const uint32_t L = ~(uint32_t)link;
  return 0x80000000u | (L & 0x07ffffffu) | ((L >> 27) << l.leaf_shift);
}
PTGS_SK_HD int32_t stack_link_unpack(uint32_t p, const StackLayout& l) {
  if (!(p & 0x80000000u)) return (int32_t)p;
  const uint32_t u = p & 0x7fffffffu;
  return (int32_t)~((u & l.leaf_start_mask) | ((u >> l.leaf_shift) << 27));
}

}  // namespace ptgs
