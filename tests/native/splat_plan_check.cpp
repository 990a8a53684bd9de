// splat_plan_check.cpp — csrc/splat_plan.h (the 3DGS forward pass's host planning) built for the host alone:
// pinned plans of the benchmark's frames, the edges of the kernels' static limits, the rule for when an `over`
// call keeps a copy of `under`, and the invariants the kernels rely on over a seeded sweep. Stand-alone (ASan + UBSan linked in by tests/test_splat_plan.py);
// prints the first failed check and exits 1.
#include <cstdio>
#include <cstdlib>

#include "splat_plan.h"

using namespace ptgs;

static int g_fail = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s | ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      if (++g_fail > 20) std::exit(1);                           \
    }                                                            \
  } while (0)

// gfx950's LDS per workgroup, and the static parts of the kernels' LDS beside the planned dynamic part
static const size_t LDS_BYTES = 160u * 1024u;
static const uint32_t SPILL_MAX = 0xFFFFFFF0u;

static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static SplatCam cam_of(uint32_t W, uint32_t H, uint32_t r0 = 0, uint32_t r1 = 0xFFFFFFFFu, bool bounds = false,
                       bool stats = false, bool publish = false, bool tight = false) {
  return gs_plan_cam(IDENT, IDENT, 1.0f, -1.7f, W, H, r0, r1, bounds, stats, publish, tight);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint64_t n) { return (uint32_t)(rnd() % n); }
// sizes spread over the orders of magnitude, edges included
static uint32_t rnd_log(uint32_t max_bits) {
  const uint32_t bits = rnd_below(max_bits + 1);
  const uint32_t v = bits == 0 ? 0u : (uint32_t)(rnd() & ((1ull << bits) - 1u));
  switch (rnd_below(8)) {
    case 0: return bits >= 32 ? 0xFFFFFFFFu : (uint32_t)(1ull << bits);
    case 1: return bits >= 32 ? 0xFFFFFFFFu : (uint32_t)((1ull << bits) - 1u);
    default: return v;
  }
}

static void check_grid_invariants(const SplatCam& cam, uint32_t n, const BinGrid& g) {
  const uint32_t rows = cam.row_end - cam.row_begin;
  CHECK(g.grid_x == cam.grid_x && g.grid_y == cam.grid_y && g.tiles == cam.grid_x * cam.grid_y, "grid");
  CHECK(g.row0 == cam.row_begin && g.row1 == cam.row_end, "rows");
  CHECK(g.band_rows >= 1 && g.bands >= 1 && g.groups >= 1, "%u %u %u", g.band_rows, g.bands, g.groups);
  CHECK((uint64_t)g.bands * g.band_rows >= rows, "bands %u x %u rows %u", g.bands, g.band_rows, rows);
  CHECK((uint64_t)(g.bands - 1) * g.band_rows < std::max(rows, 1u), "an empty band: %u x %u rows %u", g.bands, g.band_rows, rows);
  CHECK(g.band_rows * g.grid_x <= GS_BAND_TILES, "band tiles %u", g.band_rows * g.grid_x);
  CHECK((uint64_t)g.groups * 64u >= (uint64_t)rows * g.grid_x && g.groups <= GS_MAX_GROUPS, "groups %u", g.groups);
  CHECK(g.chunks >= 1 && g.chunk >= 1, "chunks %u of %u", g.chunks, g.chunk);
  CHECK((uint64_t)g.chunks * g.chunk >= n, "chunks %u of %u, n %u", g.chunks, g.chunk, n);
  // (trailing chunks may be empty, e.g. 1 024 chunks of 601 for n = 614 501: the kernels clamp a chunk to [b0, min(n, b0 + chunk)))
  CHECK(g.chunks <= GS_MAX_CHUNKS && g.bands * g.chunks <= GS_MAX_CHUNKS, "chunks %u bands %u", g.chunks, g.bands);
  // the count's histogram and the scatter's cursors + totals + group prefix fit the LDS
  const size_t band_lds = (size_t)g.band_rows * g.grid_x * 4;
  CHECK(2 * band_lds + (size_t)g.groups * 4 + 40u * 1024u <= LDS_BYTES, "scatter LDS %zu", 2 * band_lds + (size_t)g.groups * 4);
  // the fused front end's window for both shapes and every override
  for (int env : {0, 256, 512, 7})
    for (int ov = 0; ov < 2; ++ov) {
      const GsFusedPlan p = gs_plan_fused_shape(env, ov != 0, band_lds);
      const uint32_t want = env == 256 || env == 512 ? (uint32_t)env : ov ? (uint32_t)GS_FUSED_WG_OV : (uint32_t)GS_FUSED_WG;
      CHECK(p.wg == want, "wg %u env %d ov %d", p.wg, env, ov);
      CHECK(p.lds % 4 == 0 && p.lds >= GS_ORDER_BUCKETS * 4u, "lds %zu", p.lds);
      CHECK(p.lds / 4 <= std::max<size_t>(GS_BAND_TILES, GS_ORDER_BUCKETS), "window %zu entries (gs_wg_count_keep packs 13 bits)", p.lds / 4);
      CHECK(p.lds <= std::max<size_t>(band_lds, GS_ORDER_BUCKETS * 4u), "lds %zu above the band's %zu", p.lds, band_lds);
      if (p.wg == 256) CHECK(p.lds <= std::max<size_t>(GsFusedShape<256>::lds_cap, GS_ORDER_BUCKETS) * 4u, "lds %zu", p.lds);
      else CHECK(p.lds == std::max<size_t>(band_lds, GS_ORDER_BUCKETS * 4u), "lds %zu", p.lds);
    }
}

static void check_scap(int frontend, uint32_t runs, bool hint, uint32_t n, uint32_t tiles, uint32_t tile) {
  const uint32_t scap = gs_plan_scap(frontend, runs, hint, n, tiles, tile);
  if (scap == 0) {
    // three launches: asked for, no hint yet, nothing to render, an incoherent order, or rows too large
    const bool policy_three = frontend == 2 && runs > GS_FUSED_RUNS_PER_TILE * tiles;
    const uint64_t big = std::max<uint64_t>(256u, (uint64_t)tile + tile / 4u);
    uint64_t c = 256;
    while (c < big) c <<= 1;
    CHECK(frontend == 0 || !hint || n == 0 || policy_three || big > GS_FUSED_MAX_SCAP || (uint64_t)tiles * c * 8 > (4ull << 30),
          "three launches without a reason: fe %d runs %u hint %d n %u tiles %u tile %u", frontend, runs, hint, n, tiles, tile);
    return;
  }
  CHECK(frontend != 0 && hint && n != 0, "fused without a hint: fe %d hint %d n %u", frontend, hint, n);
  CHECK(frontend == 1 || runs <= GS_FUSED_RUNS_PER_TILE * tiles, "fused against the policy: runs %u tiles %u", runs, tiles);
  CHECK((scap & (scap - 1)) == 0 && scap >= 256 && scap <= GS_FUSED_MAX_SCAP, "scap %u", scap);
  CHECK((uint64_t)scap >= (uint64_t)tile + tile / 4u, "scap %u below tile %u + 1/4", scap, tile);
  CHECK(scap == 256 || scap / 2 < (uint64_t)tile + tile / 4u, "scap %u is not the smallest power for tile %u", scap, tile);
  CHECK((uint64_t)tiles * scap * 8 <= (4ull << 30), "rows of %llu bytes", (unsigned long long)tiles * scap * 8);
}

static void check_sort(uint32_t tile, uint32_t large) {
  const GsSortPlan p = gs_plan_sort(tile, large);
  const uint32_t big = tile + tile / 8u;  // (as the rule: a hint; wraps only beyond any tile)
  CHECK((p.r & 1u) == 1u && p.r >= 1 && p.r <= GS_RADIX_MAXR, "sort_r %u", p.r);
  if (tile <= 0xE0000000u && big <= GS_SORT_THREADS * GS_RADIX_MAXR)
    CHECK(p.r * GS_SORT_THREADS >= big && !gs_plan_sort_scratch(tile), "sort_r %u tile %u", p.r, tile);
  CHECK(p.grid >= 64 && p.grid <= 4096, "sort_grid %u", p.grid);
  if (large <= 3276) CHECK(p.grid >= large, "sort_grid %u below %u large tiles", p.grid, large);
  CHECK(gs_plan_sort_large(tile) == (tile > GS_MID), "sort_large");
  CHECK(gs_plan_sort_scratch(tile) == (tile > GS_SORT_THREADS * GS_RADIX_MAXR), "scratch");
  const uint32_t tiles = rnd_log(18);
  const uint32_t fg = gs_plan_sort_grid_fused(p.grid, tiles);
  CHECK(fg >= p.grid && (uint64_t)fg * GS_SORT_THREADS >= tiles, "fused sort grid %u tiles %u", fg, tiles);
}

static void check_helpers(uint32_t queued, uint32_t pairs, uint32_t owners) {
  CHECK(gs_plan_helpers(false, 0) == 0, "helpers without queued slices");
  CHECK(gs_plan_helpers(true, queued) == GS_FUSED_HELPERS, "helpers always");
  const uint32_t h = gs_plan_helpers(false, queued);
  CHECK(h <= GS_FUSED_HELPERS && (queued == 0) == (h == 0), "helpers %u queued %u", h, queued);
  if (queued && queued < GS_FUSED_HELPERS / 2) CHECK(h >= queued, "helpers %u queued %u", h, queued);
  if (owners <= 0x7FFFFFFFu) {
    const uint32_t q = gs_plan_queue_cap(pairs, owners);
    CHECK(q >= 4096 && q >= owners && q >= pairs / GsFusedShape<256>::slice, "queue %u pairs %u owners %u", q, pairs, owners);
  }
}

static void check_spill(uint32_t n, uint32_t cap, uint32_t demand, bool inc, uint32_t k) {
  const uint64_t want = gs_plan_spill_pool(n, cap, demand, inc, k);
  const uint64_t floor_ = std::max<uint64_t>(std::max<uint64_t>(1u << 20, n), cap);
  CHECK(want <= SPILL_MAX && want >= std::min<uint64_t>(floor_, SPILL_MAX), "pool %llu n %u cap %u", (unsigned long long)want, n, cap);
  if (demand > cap)
    CHECK(want >= std::min<uint64_t>((uint64_t)demand + demand / 4u, SPILL_MAX), "pool %llu demand %u", (unsigned long long)want, demand);
  if (inc) CHECK(want >= std::min<uint64_t>((uint64_t)k + k / 4u, SPILL_MAX), "pool %llu after a report, K %u", (unsigned long long)want, k);
  if (demand <= cap && !inc) CHECK(want == std::min<uint64_t>(floor_, SPILL_MAX), "pool %llu grew without demand", (unsigned long long)want);
  CHECK(gs_spill_capacity((size_t)want * 8, (size_t)want * 4) == want, "capacity of %llu", (unsigned long long)want);
}

// gs_plan_under_copy: a call with stats keeps a copy of `under` exactly when its W * H * 16 bytes overlap `out`'s
static void check_under_copy(uintptr_t under, uintptr_t out, uint32_t W, uint32_t H) {
  const uint64_t bytes = (uint64_t)W * H * 16u;
  bool overlap = false;  // (restated with 128-bit ends: no wrap at the top of the address space)
  if (under) {
    const unsigned __int128 u0 = under, u1 = u0 + bytes, o0 = out, o1 = o0 + bytes;
    overlap = u0 < o1 && o0 < u1;
  }
  const void* pu = (const void*)under;
  const void* po = (const void*)out;
  CHECK(gs_plan_under_copy(true, pu, po, W, H) == overlap, "under %llx out %llx %u x %u", (unsigned long long)under,
        (unsigned long long)out, W, H);
  CHECK(gs_plan_under_copy(true, po, pu, W, H) == (overlap && out != 0), "swapped: under %llx out %llx %u x %u",
        (unsigned long long)out, (unsigned long long)under, W, H);
  CHECK(!gs_plan_under_copy(false, pu, po, W, H), "a copy without stats");
  CHECK(!gs_plan_under_copy(true, nullptr, po, W, H) && !gs_plan_under_copy(false, nullptr, po, W, H), "a copy without `under`");
}

static void under_copy_cases() {
  const uint32_t W = 1920, H = 1080;
  const uintptr_t bytes = (uintptr_t)W * H * 16u, base = 0x7f0000000000ull;
  check_under_copy(base, base, W, H);              // in place: every hybrid caller
  check_under_copy(base, base + 16, W, H);         // one pixel apart, from either side (the check swaps them too)
  check_under_copy(base, base + bytes / 2, W, H);
  check_under_copy(base, base + bytes - 1, W, H);  // the last byte
  check_under_copy(base, base + bytes, W, H);      // adjacent: no overlap
  check_under_copy(base + bytes, base, W, H);
  check_under_copy(base, base + bytes + 16, W, H);
  check_under_copy(base, base + (1ull << 40), W, H);
  CHECK(gs_plan_under_copy(true, (const void*)base, (const void*)base, W, H), "in place");
  CHECK(gs_plan_under_copy(true, (const void*)(base + bytes - 16), (const void*)base, W, H) &&
            gs_plan_under_copy(true, (const void*)base, (const void*)(base + bytes - 16), W, H),
        "the last pixel overlaps the first, from either side");
  CHECK(!gs_plan_under_copy(true, (const void*)(base + bytes), (const void*)base, W, H) &&
            !gs_plan_under_copy(true, (const void*)base, (const void*)(base + bytes), W, H),
        "adjacent ranges");
  CHECK(!gs_plan_under_copy(false, (const void*)base, (const void*)base, W, H), "no stats: one blend, no copy");
  CHECK(!gs_plan_under_copy(true, nullptr, (const void*)base, W, H), "no `under`: a plain frame");
  CHECK(!gs_plan_under_copy(true, (const void*)base, (const void*)base, 0, H), "an empty image");
  // ranges that end at the top of the address space, and images beyond 4 GiB
  check_under_copy(~(uintptr_t)0 - bytes + 1, ~(uintptr_t)0 - 2 * bytes + 1, W, H);
  check_under_copy(~(uintptr_t)0 - 15, 16, 1, 1);
  check_under_copy(base, base + (1ull << 33), 131072, 8192);
  check_under_copy(base, base + (1ull << 34), 131072, 8192);
}

static void pinned() {
  BinGrid g;
  SplatCam cam = cam_of(1920, 1080);
  CHECK(cam.grid_x == 120 && cam.grid_y == 68 && cam.row_begin == 0 && cam.row_end == 68 && !cam.rowcull && !cam.cull && cam.tight,
        "1080p cam %u x %u", cam.grid_x, cam.grid_y);
  CHECK(gs_plan_grid(cam, 1000000u, &g), "1080p 1M");
  CHECK(g.bands == 1 && g.band_rows == 68 && g.chunks == 256 && g.chunk == 3907 && g.groups == 128 && g.tiles == 8160,
        "1080p 1M: %u bands of %u, %u chunks of %u", g.bands, g.band_rows, g.chunks, g.chunk);
  check_grid_invariants(cam, 1000000u, g);
  CHECK(gs_plan_grid(cam, 100000u, &g), "1080p 100k");
  CHECK(g.bands == 1 && g.band_rows == 68 && g.chunks == 196 && g.chunk == 511, "1080p 100k: %u bands, %u chunks of %u", g.bands,
        g.chunks, g.chunk);
  check_grid_invariants(cam, 100000u, g);
  cam = cam_of(3840, 2160);
  CHECK(cam.grid_x == 240 && cam.grid_y == 135, "4K cam %u x %u", cam.grid_x, cam.grid_y);
  CHECK(gs_plan_grid(cam, 10000000u, &g), "4K 10M");
  CHECK(g.band_rows == 34 && g.bands == 4 && g.chunks == 256 && g.chunk == 39063, "4K 10M: %u bands of %u, %u chunks of %u", g.bands,
        g.band_rows, g.chunks, g.chunk);
  check_grid_invariants(cam, 10000000u, g);
  CHECK(gs_tile_begin(cam) == 0 && gs_tile_end(cam) == 32400, "4K tiles");
  CHECK(gs_chunks256(0) == 0 && gs_chunks256(1) == 1 && gs_chunks256(256) == 1 && gs_chunks256(257) == 2, "chunks256");
  // the camera's scalars
  cam = gs_plan_cam(IDENT, IDENT, 2.0f, -3.0f, 640, 480, 0, 30, false, false, false, false);
  CHECK(cam.fx == 640.0f && cam.fy == -720.0f && cam.tan_fovx == 0.5f && cam.tan_fovy == 1.0f / 3.0f && cam.fmax2 == 720.0f * 720.0f,
        "cam scalars %g %g %g %g", cam.fx, cam.fy, cam.tan_fovx, cam.tan_fovy);
  CHECK(cam.w2 == (float)(1.0 * (1.0 + 1e-5)), "a rotation's Gershgorin bound: %g", cam.w2);
  float scaled[16];
  for (int i = 0; i < 16; ++i) scaled[i] = 2.0f * IDENT[i];
  scaled[4] = 1.0f;  // rows of W W^T: (4 + 1, 2), (2, 4): the largest row sum is 7
  cam = gs_plan_cam(scaled, IDENT, 2.0f, -3.0f, 640, 480, 0, 30, false, false, false, false);
  CHECK(cam.w2 == (float)(7.0 * (1.0 + 1e-5)) && cam.view[4] == 1.0f && cam.mvp[0] == 1.0f, "Gershgorin bound %g", cam.w2);
  // binning: the alpha box for stream-ordered frames and publish_tight, the 3-sigma rects for stats / published frames
  CHECK(cam_of(64, 64, 0, 99, false, false, false, false).tight == 1 && cam_of(64, 64, 0, 99, false, true, false, false).tight == 0 &&
            cam_of(64, 64, 0, 99, false, false, true, false).tight == 0 && cam_of(64, 64, 0, 99, false, true, true, true).tight == 1 &&
            cam_of(64, 64, 0, 99, false, true, false, true).tight == 0,
        "tight");
}

static void edges() {
  BinGrid g;
  const SplatCam hd = cam_of(1920, 1080);
  const struct { uint32_t n, chunks, chunk; } small[] = {{0, 1, 1}, {1, 1, 1}, {GS_CHUNK_MIN - 1, 1, GS_CHUNK_MIN - 1},
                                                          {GS_CHUNK_MIN, 1, GS_CHUNK_MIN}, {GS_CHUNK_MIN + 1, 2, GS_CHUNK_MIN / 2 + 1}};
  for (const auto& s : small) {
    CHECK(gs_plan_grid(hd, s.n, &g) && g.chunks == s.chunks && g.chunk == s.chunk, "n %u: %u chunks of %u", s.n, g.chunks, g.chunk);
    check_grid_invariants(hd, s.n, g);
  }
  SplatCam cam = cam_of(16, 16);
  CHECK(cam.grid_x == 1 && cam.grid_y == 1 && gs_plan_grid(cam, 1000, &g) && g.tiles == 1 && g.bands == 1 && g.band_rows == 1 && g.groups == 1,
        "16x16");
  check_grid_invariants(cam, 1000, g);
  // the two limits
  cam = cam_of(131072, 16);
  CHECK(cam.grid_x == GS_BAND_TILES && gs_plan_grid(cam, 1000, &g) && g.band_rows == 1 && g.bands == 1, "W = 131072");
  check_grid_invariants(cam, 1000, g);
  CHECK(!gs_plan_grid(cam_of(131073, 16), 1000, &g), "W = 131073 accepted");
  cam = cam_of(8192, 8192);
  CHECK(gs_plan_grid(cam, 5000000, &g) && g.groups == GS_MAX_GROUPS && g.band_rows == 16 && g.bands == 32, "8192x8192: %u groups", g.groups);
  check_grid_invariants(cam, 5000000, g);
  CHECK(!gs_plan_grid(cam_of(8192, 8208), 1000, &g), "8192x8208 accepted");
  // tile rows: beyond the grid, and an empty range
  cam = cam_of(1920, 1080, 100, 200, true);
  CHECK(cam.row_begin == 68 && cam.row_end == 68 && cam.rowcull && cam.cull, "rows beyond the grid: %u %u", cam.row_begin, cam.row_end);
  CHECK(gs_plan_grid(cam, 100000, &g) && g.groups == 1 && g.band_rows == 1 && g.bands == 1, "rows beyond the grid: plan");
  check_grid_invariants(cam, 100000, g);
  cam = cam_of(1920, 1080, 40, 10);
  CHECK(cam.row_begin == 40 && cam.row_end == 40 && cam.rowcull && !cam.cull, "row_end < row_begin: %u %u", cam.row_begin, cam.row_end);
  CHECK(gs_plan_grid(cam, 100000, &g) && g.groups >= 1 && g.band_rows >= 1 && g.bands >= 1 && g.row0 == g.row1, "an empty frame's plan");
  check_grid_invariants(cam, 100000, g);
  CHECK(gs_tile_begin(cam) == gs_tile_end(cam), "an empty frame's tiles");
  // a tile-row shard: one band of its rows, chunk bounds in use
  cam = cam_of(3840, 2160, 34, 68, true);
  CHECK(cam.rowcull && cam.cull && gs_plan_grid(cam, 10000000u, &g) && g.bands == 1 && g.band_rows == 34 && g.chunks == 1024 &&
            g.row0 == 34 && g.row1 == 68 && g.groups == 128,
        "4K shard: %u bands of %u, %u chunks", g.bands, g.band_rows, g.chunks);
  check_grid_invariants(cam, 10000000u, g);
  CHECK(gs_tile_begin(cam) == 34 * 240 && gs_tile_end(cam) == 68 * 240, "shard tiles");
  // scap: thresholds
  CHECK(gs_plan_scap(2, 0, true, 1000, 8160, 0) == 256 && gs_plan_scap(2, 0, true, 1000, 8160, 205) == 256 &&
            gs_plan_scap(2, 0, true, 1000, 8160, 206) == 512 && gs_plan_scap(2, 0, true, 1000, 8160, 1639) == 2048 &&
            gs_plan_scap(2, 0, true, 1000, 8160, 1640) == 0,
        "scap steps");
  CHECK(gs_plan_scap(2, 32 * 8160, true, 1000, 8160, 300) == 512 && gs_plan_scap(2, 32 * 8160 + 1, true, 1000, 8160, 300) == 0 &&
            gs_plan_scap(1, 0xFFFFFFFFu, true, 1000, 8160, 300) == 512 && gs_plan_scap(0, 0, true, 1000, 8160, 300) == 0 &&
            gs_plan_scap(1, 0, false, 1000, 8160, 300) == 0 && gs_plan_scap(1, 0, true, 0, 8160, 300) == 0,
        "front-end choice");
  CHECK(gs_plan_scap(1, 0, true, 1000, 262144, 1600) == 2048 && gs_plan_scap(1, 0, true, 1000, 262145, 1600) == 0, "rows above 4 GiB");
  // the sort's shape at the LDS limit
  CHECK(gs_plan_sort(0, 0).r == 1 && gs_plan_sort(0, 0).grid == 64 && gs_plan_sort(7509, 4000).r == 33 && gs_plan_sort(7509, 4000).grid == 4096 &&
            gs_plan_sort(100000, 100).r == GS_RADIX_MAXR && gs_plan_sort(2048, 100).r == 9 && gs_plan_sort(2048, 100).grid == 125,
        "sort shapes");
  CHECK(!gs_plan_sort_large(512) && gs_plan_sort_large(513) && !gs_plan_sort_scratch(8448) && gs_plan_sort_scratch(8449), "sort thresholds");
  CHECK(gs_plan_helpers(false, 1) == 9 && gs_plan_helpers(false, 80) == 128 && gs_plan_helpers(false, 79) == 126, "helper steps");
  CHECK(gs_plan_queue_cap(0, 0) == 4096 && gs_plan_queue_cap(617000, 2344) == 4096 &&
            gs_plan_queue_cap(10000000, 39063) == 2 * 4882 + 39063,
        "queue cap");
  check_spill(0, 0, 0, false, 0);
  check_spill(0xFFFFFFFFu, 0, 0xFFFFFFFFu, true, 0xFFFFFFFFu);
  CHECK(gs_plan_spill_pool(1000, 0, 0, false, 0) == (1u << 20) && gs_plan_spill_pool(3000000, 0, 0, false, 0) == 3000000 &&
            gs_plan_spill_pool(1000, 1u << 20, (1u << 20) + 4, false, 0) == (1u << 20) + 4 + (1u << 18) + 1 &&
            gs_plan_spill_pool(1000, 1u << 20, 4, true, 4000000) == 5000000 && gs_plan_spill_pool(1000, 1u << 20, 4, false, 4000000) == (1u << 20),
        "spill pool");
}

static void sweep(uint32_t rounds) {
  BinGrid g;
  uint32_t accepted = 0;
  for (uint32_t i = 0; i < rounds; ++i) {
    // images: mostly the sizes frames have, some up to the limits and beyond
    const uint32_t mode = rnd_below(8);
    const uint32_t W = mode < 5 ? 1 + rnd_below(4096) : mode < 7 ? 1 + rnd_below(16384) : 1 + rnd_log(18);
    const uint32_t H = mode < 5 ? 1 + rnd_below(2400) : mode < 7 ? 1 + rnd_below(16384) : 1 + rnd_log(15);
    const uint32_t gy = (H + 15) / 16;
    uint32_t r0 = 0, r1 = 0xFFFFFFFFu;
    if (rnd_below(2)) {
      r0 = rnd_below(gy + 3);
      r1 = rnd_below(4) ? r0 + rnd_below(gy + 2) : rnd_below(gy + 3);
    }
    // (n up to 2^31: the rules round n up in 32-bit arithmetic, and a set takes 59 bytes per Gaussian)
    const uint32_t n = rnd_below(4) ? rnd_log(25) : rnd_log(31);
    const bool bounds = rnd_below(2) != 0, stats = rnd_below(2) != 0, publish = rnd_below(2) != 0, tight = rnd_below(2) != 0;
    const SplatCam cam = cam_of(W, H, r0, r1, bounds, stats, publish, tight);
    CHECK(cam.grid_x == (W + 15) / 16 && cam.grid_y == gy && cam.W == W && cam.H == H, "cam grid");
    CHECK(cam.row_begin <= cam.row_end && cam.row_end <= cam.grid_y && cam.row_begin == std::min(r0, gy), "cam rows %u %u", cam.row_begin, cam.row_end);
    if (r1 >= r0) CHECK(cam.row_end == std::min(r1, gy), "cam row_end %u", cam.row_end);
    CHECK(cam.rowcull == (cam.row_begin > 0 || cam.row_end < gy ? 1u : 0u) && cam.cull == (bounds && cam.rowcull ? 1u : 0u), "cam culls");
    CHECK(cam.tight == (((!stats && !publish) || (publish && tight)) ? 1u : 0u), "cam tight");
    {  // `under` at random distances from `out`, around the image's size
      const uint64_t bytes = (uint64_t)W * H * 16u;
      const uintptr_t u = (uintptr_t)(0x100000000000ull + (rnd() & 0xFFFFFFFFFF0ull));
      const uint64_t dist = rnd_below(4) ? rnd() % (2 * bytes + 16) : bytes + rnd_below(3) - 1;
      check_under_copy(u, rnd_below(2) ? u + (uintptr_t)dist : u - (uintptr_t)dist, W, H);
    }
    const bool ok = gs_plan_grid(cam, n, &g);
    const uint64_t tiles = (uint64_t)cam.grid_x * cam.grid_y;
    CHECK(ok == (cam.grid_x <= GS_BAND_TILES && (tiles + 63) / 64 <= GS_MAX_GROUPS), "accepted %d: %u x %u tiles", ok, cam.grid_x, cam.grid_y);
    if (ok) {
      ++accepted;
      check_grid_invariants(cam, n, g);
      CHECK(gs_tile_begin(cam) <= gs_tile_end(cam) && gs_tile_end(cam) <= g.tiles, "tile range");
      CHECK((uint64_t)gs_chunks256(n) * 256u >= n && (uint64_t)gs_chunks256(n) * 256u < (uint64_t)n + 256u, "chunks256 of %u", n);
      // (the hinted tile up to 2^31 pairs: the rule's tile + tile / 4 is 32-bit arithmetic, and K itself is)
      check_scap((int)rnd_below(3), rnd_below(2) ? rnd_log(32) : rnd_below(64) * (uint32_t)tiles, rnd_below(4) != 0, n, (uint32_t)tiles,
                 rnd_below(4) ? rnd_log(12) : rnd_log(31));
    }
    check_sort(rnd_below(4) ? rnd_log(15) : rnd_log(32), rnd_below(4) ? rnd_log(14) : rnd_log(31));
    check_helpers(rnd_below(3) ? rnd_log(9) : rnd_log(32), rnd_log(32), rnd_log(31));
    const uint32_t cap = std::min(rnd_log(32), SPILL_MAX);
    check_spill(n, cap, rnd_below(2) ? rnd_log(32) : cap + rnd_below(3) - 1u, rnd_below(2) != 0, rnd_log(32));
  }
  CHECK(accepted > rounds / 2, "the sweep planned only %u of %u frames", accepted, rounds);
}

int main(int argc, char** argv) {
  const uint32_t rounds = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 200000u;
  pinned();
  edges();
  under_copy_cases();
  sweep(rounds);
  if (g_fail) return 1;
  std::printf("ok: %u sweep rounds\n", rounds);
  return 0;
}
