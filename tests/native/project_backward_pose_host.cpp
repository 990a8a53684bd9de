// Host driver of the projection backward with the camera-pose term (csrc/splat_backward_math.h, DEPTH = true,
// POSE = true), for tests/test_splat_pose_grad_ref.py:
//   project_backward_pose_host IN OUT
// IN: GbCam, proj (16 floats, column-major), u32 n, then per Gaussian 16 floats (mean 3, scale 3, rotation 4,
// dL/d means2d 2, dL/d conic 3, dL/d(1/d) 1); OUT: per Gaussian 22 floats (dL/d mean 3, scale 3, rotation 4, then
// the Gaussian's twelve shares of dL/d view, [r * 4 + c] for r < 3). The shares are also printed, one Gaussian
// per line. No device code.
#include <cstdio>
#include <vector>

#include "splat_backward_math.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  ptgs::GbCam cam;
  float proj[16];
  uint32_t n = 0;
  if (fread(&cam, sizeof(cam), 1, f) != 1 || fread(proj, 4, 16, f) != 16 || fread(&n, 4, 1, f) != 1 || n > (1u << 24))
    return 4;
  std::vector<float> in((size_t)n * 16), out((size_t)n * 22);
  if (fread(in.data(), 4, in.size(), f) != in.size()) return 4;
  fclose(f);
  for (uint32_t i = 0; i < n; ++i) {
    const float* p = &in[(size_t)16 * i];
    float* o = &out[(size_t)22 * i];
    ptgs::gs_project_backward_one<true, true>(cam, p, p + 3, p + 6, p[10], p[11], p[12], p[13], p[14], o, o + 3, o + 6,
                                              p[15], proj, o + 10);
    for (int k = 0; k < 12; ++k) printf("%.9g%c", o[10 + k], k == 11 ? '\n' : ' ');
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 5;
  fclose(f);
  return 0;
}
