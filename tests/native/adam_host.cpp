// Host driver of the optimizer step (csrc/splat_adam_math.h), for tests/test_adam_ref.py:
//   adam_host layout          prints sizeof and the field offsets of the two structs of ptgs.h
//   adam_host step IN OUT     `steps` consecutive Adam steps (step, step + 1, ...) on the same gradients
//   adam_host reset IN OUT    the opacity reset
// step IN (tests/adam_ref.py pack()): u32 n, n_rows, step, steps, has_radii; f32 beta1, beta2, eps; per row u32
// width, head and f32 lr, lr_head; radii (n int32) when has_radii; per row param, grad, exp_avg, exp_avg_sq
// (n * width each). OUT: per row param, exp_avg, exp_avg_sq.
// reset IN: u32 n, has_exp_avg, has_exp_avg_sq; f32 max_opacity; logits (n); the moments that are given (n each).
// OUT: logits, then the moments that were given.
// No device code.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "splat_adam_math.h"

static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool wr(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

static int layout() {
  printf("ptgs_adam_rows %zu param %zu grad %zu exp_avg %zu exp_avg_sq %zu width %zu head %zu lr %zu lr_head %zu\n",
         sizeof(ptgs_adam_rows), offsetof(ptgs_adam_rows, param), offsetof(ptgs_adam_rows, grad),
         offsetof(ptgs_adam_rows, exp_avg), offsetof(ptgs_adam_rows, exp_avg_sq), offsetof(ptgs_adam_rows, width),
         offsetof(ptgs_adam_rows, head), offsetof(ptgs_adam_rows, lr), offsetof(ptgs_adam_rows, lr_head));
  printf("ptgs_adam_params %zu beta1 %zu beta2 %zu eps %zu step %zu\n", sizeof(ptgs_adam_params),
         offsetof(ptgs_adam_params, beta1), offsetof(ptgs_adam_params, beta2), offsetof(ptgs_adam_params, eps),
         offsetof(ptgs_adam_params, step));
  return 0;
}

static int step(const char* in, const char* out) {
  using namespace ptgs;
  FILE* f = fopen(in, "rb");
  if (!f) return 3;
  uint32_t hdr[5];
  float sc[3];
  if (!rd(f, hdr, sizeof(hdr)) || !rd(f, sc, sizeof(sc))) return 4;
  const uint32_t n = hdr[0], n_rows = hdr[1], step0 = hdr[2], steps = hdr[3], has_radii = hdr[4];
  if (n > (1u << 24) || n_rows == 0 || n_rows > PTGS_ADAM_MAX_ROWS || step0 == 0 || steps > 64) return 4;
  std::vector<uint32_t> width(n_rows), head(n_rows);
  std::vector<float> lr(n_rows), lr_head(n_rows);
  for (uint32_t k = 0; k < n_rows; ++k) {
    uint32_t wh[2];
    float ll[2];
    if (!rd(f, wh, sizeof(wh)) || !rd(f, ll, sizeof(ll)) || wh[0] == 0 || wh[0] > 4096 || wh[1] > wh[0]) return 4;
    width[k] = wh[0];
    head[k] = wh[1];
    lr[k] = ll[0];
    lr_head[k] = ll[1];
  }
  const size_t N = n;
  std::vector<int32_t> radii(has_radii ? N : 0);
  if (!rd(f, radii.data(), radii.size() * 4)) return 4;
  std::vector<std::vector<float>> p(n_rows), g(n_rows), m(n_rows), v(n_rows);
  for (uint32_t k = 0; k < n_rows; ++k)
    for (std::vector<float>* a : {&p[k], &g[k], &m[k], &v[k]}) {
      a->resize(N * width[k]);
      if (!rd(f, a->data(), a->size() * 4)) return 4;
    }
  fclose(f);
  for (uint32_t t = 0; t < steps; ++t) {
    ptgs_adam_params prm;
    prm.beta1 = sc[0];
    prm.beta2 = sc[1];
    prm.eps = sc[2];
    prm.step = step0 + t;
    float bc1 = 0.0f;
    const AdamScalars s = adam_scalars(prm, &bc1);
    for (uint32_t k = 0; k < n_rows; ++k) {
      const float ss = adam_step_size(lr[k], bc1), ss_head = adam_step_size(lr_head[k], bc1);
      for (size_t i = 0; i < N; ++i) {
        if (has_radii && radii[i] <= 0) continue;
        for (uint32_t c = 0; c < width[k]; ++c) {
          const size_t e = i * width[k] + c;
          adam_update(s, c < head[k] ? ss_head : ss, g[k][e], &p[k][e], &m[k][e], &v[k][e]);
        }
      }
    }
  }
  f = fopen(out, "wb");
  if (!f) return 5;
  bool ok = true;
  for (uint32_t k = 0; k < n_rows; ++k)
    for (std::vector<float>* a : {&p[k], &m[k], &v[k]}) ok = ok && wr(f, a->data(), a->size() * 4);
  fclose(f);
  return ok ? 0 : 5;
}

static int reset(const char* in, const char* out) {
  using namespace ptgs;
  FILE* f = fopen(in, "rb");
  if (!f) return 3;
  uint32_t hdr[3];
  float max_opacity;
  if (!rd(f, hdr, sizeof(hdr)) || !rd(f, &max_opacity, 4) || hdr[0] > (1u << 24)) return 4;
  const size_t N = hdr[0];
  std::vector<float> x(N), m(hdr[1] ? N : 0), v(hdr[2] ? N : 0);
  if (!rd(f, x.data(), N * 4) || !rd(f, m.data(), m.size() * 4) || !rd(f, v.data(), v.size() * 4)) return 4;
  fclose(f);
  const float cap = adam_reset_cap(max_opacity);
  for (size_t i = 0; i < N; ++i) x[i] = adam_reset_logit(x[i], cap);
  for (float& a : m) a = 0.0f;
  for (float& a : v) a = 0.0f;
  f = fopen(out, "wb");
  if (!f) return 5;
  const bool ok = wr(f, x.data(), N * 4) && wr(f, m.data(), m.size() * 4) && wr(f, v.data(), v.size() * 4);
  fclose(f);
  return ok ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 4 && !strcmp(argv[1], "step")) return step(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "reset")) return reset(argv[2], argv[3]);
  return 2;
}
