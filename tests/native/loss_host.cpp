// loss_host.cpp — the whole L1 + D-SSIM loss and its gradient on the host, in f32 and separably, with the
// functions of csrc/splat_loss_math.h (what splat_loss.hip's kernels evaluate per pixel). File in, file out:
//   in : u32 H, W, C; f32 lambda, grad_scale; image [H, W, 4] f32; target [H, W, C] f32
//   out: f32 loss, l1, ssim, 0; grad [H, W, 4] f32
// Built stand-alone with -fsanitize=address,undefined by tests/test_loss_ref.py.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "splat_loss_math.h"

using namespace ptgs;

namespace {

// conv(x) of one H x W plane: rows, then columns, through a zero-padded copy
std::vector<float> conv(const std::vector<float>& x, uint32_t H, uint32_t W) {
  const uint32_t PW = W + 2 * LOSS_HALO, PH = H + 2 * LOSS_HALO;
  std::vector<float> pad((size_t)PH * PW, 0.0f), rows((size_t)PH * W, 0.0f), out((size_t)H * W);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t c = 0; c < W; ++c) pad[(size_t)(y + LOSS_HALO) * PW + c + LOSS_HALO] = x[(size_t)y * W + c];
  for (uint32_t y = 0; y < PH; ++y)
    for (uint32_t c = 0; c < W; ++c) rows[(size_t)y * W + c] = loss_tap11(&pad[(size_t)y * PW + c]);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t c = 0; c < W; ++c) out[(size_t)y * W + c] = loss_tap11(&rows[(size_t)y * W + c], (int)W);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "window") {  // the eleven literals, as printf %a
    for (int k = 0; k < LOSS_WIN; ++k) printf("%a\n", (double)loss_window(k));
    return 0;
  }
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t hdr[3];
  float par[2];
  if (fread(hdr, 4, 3, f) != 3 || fread(par, 4, 2, f) != 2) return 4;
  const uint32_t H = hdr[0], W = hdr[1], C = hdr[2];
  const float lambda = par[0], grad_scale = par[1];
  if (!H || !W || (C != 3 && C != 4)) return 5;
  const size_t px = (size_t)H * W;
  std::vector<float> image(px * 4), target(px * C);
  if (fread(image.data(), 4, image.size(), f) != image.size()) return 6;
  if (fread(target.data(), 4, target.size(), f) != target.size()) return 7;
  fclose(f);

  const double n = 3.0 * (double)px;
  const float k1 = (float)((double)grad_scale * (1.0 - (double)lambda) / n);
  const float k2 = (float)((double)grad_scale * (double)lambda / n);
  std::vector<float> grad(px * 4, 0.0f);
  double sum_l1 = 0.0, sum_m = 0.0;
  for (uint32_t c = 0; c < 3; ++c) {
    std::vector<float> a(px), b(px), aa(px), bb(px), ab(px);
    for (size_t p = 0; p < px; ++p) {
      a[p] = image[4 * p + c];
      b[p] = target[C * p + c];
      aa[p] = a[p] * a[p];
      bb[p] = b[p] * b[p];
      ab[p] = a[p] * b[p];
      sum_l1 += (double)fabsf(a[p] - b[p]);
    }
    const std::vector<float> mu1 = conv(a, H, W), mu2 = conv(b, H, W), e11 = conv(aa, H, W), e22 = conv(bb, H, W),
                             e12 = conv(ab, H, W);
    std::vector<float> d_mu1(px), d_s1(px), d_s12(px);
    for (size_t p = 0; p < px; ++p) {
      const LossPixel q = loss_ssim_pixel(mu1[p], mu2[p], e11[p], e22[p], e12[p]);
      sum_m += (double)q.m;
      d_mu1[p] = q.d_mu1;
      d_s1[p] = q.d_s1;
      d_s12[p] = q.d_s12;
    }
    const std::vector<float> g0 = conv(d_mu1, H, W), g1 = conv(d_s1, H, W), g2 = conv(d_s12, H, W);
    for (size_t p = 0; p < px; ++p) {
      const float G = fmaf(b[p], g2[p], fmaf(2.0f * a[p], g1[p], g0[p]));
      grad[4 * p + c] = k1 * loss_sign(a[p] - b[p]) - k2 * G;
    }
  }
  const double l1 = sum_l1 / n, ssim = sum_m / n, lam = (double)lambda;
  const float terms[4] = {(float)((1.0 - lam) * l1 + lam * (1.0 - ssim)), (float)l1, (float)ssim, 0.0f};
  f = fopen(argv[2], "wb");
  if (!f) return 8;
  fwrite(terms, 4, 4, f);
  fwrite(grad.data(), 4, grad.size(), f);
  fclose(f);
  return 0;
}
