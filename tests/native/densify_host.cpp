// Host driver of densification and pruning (csrc/splat_densify_math.h), for tests/test_densify_ref.py:
//   densify_host layout          prints sizeof and the field offsets of the three structs of ptgs.h
//   densify_host IN OUT          accumulate, plan and apply, serially, through the header's functions
// IN (tests/densify_ref.py pack()): u32 n, n_rows, then (width, zero_new) per row; the five thresholds; means
// (3 n), log_scales (3 n), rotations (4 n), scales (3 n), opacities, accum, denom, max_radii (n each), noise (6 n),
// the rows; then u32 views and per view u32 W, H, g2d (2 n), radii (n, int32): the statistic of those views is
// accumulated from zero, apart from the plan's.
// OUT: u32 survivors, clones, split_sources, pruned_originals, pruned_children, total; source (total u32);
// means' (3 total); log_scales' (3 total); each row's output; then the views' accum, denom, max_radii (n each).
// No device code.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "splat_densify_math.h"

static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool wr(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

static int layout() {
  printf("ptgs_densify_params %zu grad_threshold %zu scale_split %zu min_opacity %zu max_scale %zu max_screen_radius %zu\n",
         sizeof(ptgs_densify_params), offsetof(ptgs_densify_params, grad_threshold),
         offsetof(ptgs_densify_params, scale_split), offsetof(ptgs_densify_params, min_opacity),
         offsetof(ptgs_densify_params, max_scale), offsetof(ptgs_densify_params, max_screen_radius));
  printf("ptgs_densify_counts %zu survivors %zu clones %zu split_sources %zu pruned_originals %zu pruned_children %zu total %zu\n",
         sizeof(ptgs_densify_counts), offsetof(ptgs_densify_counts, survivors), offsetof(ptgs_densify_counts, clones),
         offsetof(ptgs_densify_counts, split_sources), offsetof(ptgs_densify_counts, pruned_originals),
         offsetof(ptgs_densify_counts, pruned_children), offsetof(ptgs_densify_counts, total));
  printf("ptgs_densify_rows %zu src %zu dst %zu width %zu zero_new %zu\n", sizeof(ptgs_densify_rows),
         offsetof(ptgs_densify_rows, src), offsetof(ptgs_densify_rows, dst), offsetof(ptgs_densify_rows, width),
         offsetof(ptgs_densify_rows, zero_new));
  return 0;
}

int main(int argc, char** argv) {
  using namespace ptgs;
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t hdr[2];
  if (!rd(f, hdr, sizeof(hdr))) return 4;
  const uint32_t n = hdr[0], n_rows = hdr[1];
  if (n > DN_MAX_N || n_rows > PTGS_DENSIFY_MAX_ROWS) return 4;
  std::vector<uint32_t> width(n_rows), zero_new(n_rows);
  for (uint32_t k = 0; k < n_rows; ++k) {
    uint32_t wz[2];
    if (!rd(f, wz, sizeof(wz)) || wz[0] == 0 || wz[0] > 4096) return 4;
    width[k] = wz[0];
    zero_new[k] = wz[1];
  }
  ptgs_densify_params p;
  if (!rd(f, &p, sizeof(p))) return 4;
  const size_t N = n;
  std::vector<float> means(3 * N), log_scales(3 * N), rot(4 * N), scales(3 * N), opac(N), accum(N), denom(N), maxr(N),
      noise(6 * N);
  for (std::vector<float>* v : {&means, &log_scales, &rot, &scales, &opac, &accum, &denom, &maxr, &noise})
    if (!rd(f, v->data(), v->size() * 4)) return 4;
  std::vector<std::vector<float>> rows(n_rows);
  for (uint32_t k = 0; k < n_rows; ++k) {
    rows[k].resize(N * width[k]);
    if (!rd(f, rows[k].data(), rows[k].size() * 4)) return 4;
  }
  // ---- the statistic of the views, from zero ----
  std::vector<float> vaccum(N, 0.0f), vdenom(N, 0.0f), vmaxr(N, 0.0f);
  uint32_t views = 0;
  if (!rd(f, &views, 4) || views > 64) return 4;
  for (uint32_t v = 0; v < views; ++v) {
    uint32_t wh[2];
    std::vector<float> g2d(2 * N);
    std::vector<int32_t> radii(N);
    if (!rd(f, wh, sizeof(wh)) || !rd(f, g2d.data(), g2d.size() * 4) || !rd(f, radii.data(), radii.size() * 4)) return 4;
    for (size_t i = 0; i < N; ++i)
      if (radii[i] > 0) dn_accumulate_one(g2d[2 * i], g2d[2 * i + 1], radii[i], wh[0], wh[1], &vaccum[i], &vdenom[i], &vmaxr[i]);
  }
  fclose(f);
  // ---- plan: the decision, then the four runs of the source map, each by source index ----
  std::vector<uint8_t> fate(N);
  uint32_t cnt[DN_FATES] = {};
  for (size_t i = 0; i < N; ++i) {
    const uint32_t b = dn_decide(p, &scales[3 * i], opac[i], accum[i], denom[i], maxr[i]);
    fate[i] = (uint8_t)b;
    for (int k = 0; k < DN_FATES; ++k) cnt[k] += (b >> k) & 1u;
  }
  std::vector<uint32_t> source;
  const uint32_t pass_bit[4] = {DN_KEEP, DN_CLONE, DN_CHILDREN, DN_CHILDREN};
  for (uint32_t kind = 0; kind < 4; ++kind)
    for (size_t i = 0; i < N; ++i)
      if (fate[i] & pass_bit[kind]) source.push_back((uint32_t)i | (kind << DN_KIND_SHIFT));
  const uint32_t total = cnt[0] + cnt[1] + 2 * cnt[2];
  if (source.size() != total) return 6;
  // ---- apply ----
  const size_t T = total;
  std::vector<float> means_out(3 * T), ls_out(3 * T);
  std::vector<std::vector<float>> outs(n_rows);
  for (uint32_t k = 0; k < n_rows; ++k) outs[k].resize(T * width[k]);
  for (size_t o = 0; o < T; ++o) {
    const uint32_t kind = source[o] >> DN_KIND_SHIFT;
    const size_t i = source[o] & DN_INDEX_MASK;
    if (i >= N) return 6;
    for (int c = 0; c < 3; ++c) {
      means_out[3 * o + c] = means[3 * i + c];
      ls_out[3 * o + c] = kind >= DN_KIND_CHILD0 ? log_scales[3 * i + c] - DN_LOG_SPLIT : log_scales[3 * i + c];
    }
    if (kind >= DN_KIND_CHILD0)
      dn_child_mean(&means[3 * i], &rot[4 * i], &scales[3 * i], &noise[((size_t)(kind - DN_KIND_CHILD0) * N + i) * 3],
                    &means_out[3 * o]);
    for (uint32_t k = 0; k < n_rows; ++k)
      for (uint32_t c = 0; c < width[k]; ++c)
        outs[k][o * width[k] + c] = zero_new[k] && kind != DN_KIND_ORIGINAL ? 0.0f : rows[k][i * width[k] + c];
  }
  f = fopen(argv[2], "wb");
  if (!f) return 5;
  const uint32_t counts[6] = {cnt[0], cnt[1], cnt[2], cnt[3], 2 * cnt[4], total};
  bool ok = wr(f, counts, sizeof(counts)) && wr(f, source.data(), T * 4) && wr(f, means_out.data(), means_out.size() * 4) &&
            wr(f, ls_out.data(), ls_out.size() * 4);
  for (uint32_t k = 0; k < n_rows; ++k) ok = ok && wr(f, outs[k].data(), outs[k].size() * 4);
  ok = ok && wr(f, vaccum.data(), N * 4) && wr(f, vdenom.data(), N * 4) && wr(f, vmaxr.data(), N * 4);
  fclose(f);
  return ok ? 0 : 5;
}
