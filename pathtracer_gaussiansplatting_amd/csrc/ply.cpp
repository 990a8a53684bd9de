// ply.cpp — PLY point-cloud reader for the 3DGS initialisation. Reads the vertex
// element of what Engine::savePly writes (ASCII, "x y z nx ny nz red green blue" with float / uchar
// properties, engine.cpp:2849-2895) and the binary little / big endian variants other tools write.
// Properties are matched by name: x y z (required), nx ny nz, red green blue (uchar, or float in
// [0, 1] scaled by 255 and rounded); a trained-3DGS file without rgb gives colours from its SH DC
// term f_dc_0..2 (0.5 + C0 * f_dc, clamped). Elements before "vertex" must have fixed-size rows in
// binary files (list properties are only skippable in ASCII).
// ptgs_read_gaussian_ply reads the whole of such a trained-3DGS file (means, log-scales, rotations,
// opacity logits, SH coefficients) through the same header and row parsing; ptgs_write_gaussian_ply, at the
// end, writes one (binary little endian, the trainer's property order).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ptgs/ptgs_host.h"
#include "image_decode.h"

namespace {

struct Prop {
  std::string name, type;
  bool list = false;
  int size = 0;
};
struct Elem {
  std::string name;
  uint64_t count = 0;
  std::vector<Prop> props;
};

int type_size(const std::string& t) {
  if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
  if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
  if (t == "int" || t == "uint" || t == "int32" || t == "uint32" || t == "float" || t == "float32") return 4;
  if (t == "double" || t == "float64") return 8;
  return 0;
}

double read_bin(const uint8_t* p, const std::string& t, bool big) {
  uint8_t b[8];
  int n = type_size(t);
  for (int i = 0; i < n; ++i) b[i] = big ? p[n - 1 - i] : p[i];
  if (t == "char" || t == "int8") return (int8_t)b[0];
  if (t == "uchar" || t == "uint8") return b[0];
  if (t == "short" || t == "int16") { int16_t v; memcpy(&v, b, 2); return v; }
  if (t == "ushort" || t == "uint16") { uint16_t v; memcpy(&v, b, 2); return v; }
  if (t == "int" || t == "int32") { int32_t v; memcpy(&v, b, 4); return v; }
  if (t == "uint" || t == "uint32") { uint32_t v; memcpy(&v, b, 4); return v; }
  if (t == "float" || t == "float32") { float v; memcpy(&v, b, 4); return v; }
  double v;
  memcpy(&v, b, 8);
  return v;
}

bool is_float_type(const std::string& t) { return t == "float" || t == "float32" || t == "double" || t == "float64"; }

uint8_t to_u8(double v, bool is_float) {
  if (is_float) v = std::floor(v * 255.0 + 0.5);
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// A PLY file with its header parsed and its element sizes checked against the body.
struct PlyFile {
  std::vector<uint8_t> bytes;
  std::vector<Elem> elems;
  int vi = -1;  // the "vertex" element
  bool ascii = false, big = false;
  size_t hdr_end = 0, vert_off = 0, vert_rs = 0;  // binary: offset and row size of the vertex rows
  const Elem& vertex() const { return elems[vi]; }
};

// Reads `path`, parses the header and checks that the header's counts fit the body. PTGS_OK: f.vertex()
// is the vertex element (count <= 2^32 - 1, at least one property).
int ply_open(const char* path, PlyFile& f) {
  std::vector<uint8_t>& bytes = f.bytes;
  if (!ptgs::read_file(path, bytes)) return PTGS_EIO;
  // header
  size_t hdr_end = 0;
  {
    const char* tag = "end_header";
    const char* s = (const char*)bytes.data();
    size_t n = bytes.size();
    for (size_t i = 0; i + 10 <= n; ++i)
      if (!memcmp(s + i, tag, 10)) {
        size_t j = i + 10;
        while (j < n && s[j] != '\n') ++j;
        hdr_end = std::min(j + 1, n);  // (a header that ends the file without a newline)
        break;
      }
  }
  if (!hdr_end || bytes.size() < 4 || memcmp(bytes.data(), "ply", 3)) return PTGS_EIO;
  std::istringstream hs(std::string((const char*)bytes.data(), hdr_end));
  std::string line, fmt;
  std::vector<Elem>& elems = f.elems;
  while (std::getline(hs, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream ls(line);
    std::string kw;
    ls >> kw;
    if (kw == "format") {
      ls >> fmt;
    } else if (kw == "element") {
      Elem e;
      ls >> e.name >> e.count;
      elems.push_back(e);
    } else if (kw == "property") {
      if (elems.empty()) return PTGS_EIO;
      Prop p;
      std::string t;
      ls >> t;
      if (t == "list") {  // "list <count type> <item type> <name>": ASCII only
        std::string ct, it;
        ls >> ct >> it >> p.name;
        p.list = true;
        p.type = it;
      } else {
        p.type = t;
        ls >> p.name;
        p.size = type_size(t);
        if (!p.size) return PTGS_EIO;
      }
      elems.back().props.push_back(p);
    }
  }
  const bool ascii = fmt == "ascii", big = fmt == "binary_big_endian";
  if (!ascii && fmt != "binary_little_endian" && !big) return PTGS_EIO;
  int vi = -1;
  for (size_t i = 0; i < elems.size(); ++i)
    if (elems[i].name == "vertex") { vi = (int)i; break; }
  if (vi < 0) return PTGS_EIO;
  const Elem& V = elems[vi];
  if (V.count > 0xFFFFFFFFull) return PTGS_ERANGE;
  if (V.props.empty()) return PTGS_EIO;  // (rows of no bytes: the count would be unbounded)
  // header counts must fit the body (checked before the count query returns, so a caller never
  // sizes buffers from an impossible count): ASCII rows take at least one byte each, binary rows
  // exactly their size (elements before "vertex" must have fixed-size rows)
  const uint64_t body = bytes.size() - std::min(hdr_end, bytes.size());
  size_t vert_off = hdr_end, vert_rs = 0;
  if (ascii) {
    for (int e = 0; e <= vi; ++e)
      if (elems[e].count > body) return PTGS_EIO;
  } else {
    for (int e = 0; e <= vi; ++e) {
      size_t rs = 0;
      for (const Prop& pr : elems[e].props) {
        if (pr.list) return PTGS_EIO;  // variable-size rows: unsupported in binary
        rs += (size_t)pr.size;
      }
      const size_t left = bytes.size() - std::min(vert_off, bytes.size());
      if (rs && elems[e].count > left / rs) return PTGS_EIO;  // (overflow-free)
      if (e == vi) vert_rs = rs;
      else vert_off += rs * elems[e].count;
    }
  }
  f.vi = vi;
  f.ascii = ascii;
  f.big = big;
  f.hdr_end = hdr_end;
  f.vert_off = vert_off;
  f.vert_rs = vert_rs;
  return PTGS_OK;
}

// Decodes the vertex rows one by one into `row` (one double per property, list properties 0) and calls
// emit(i) after each.
template <typename Emit>
int ply_vertex_rows(PlyFile& f, std::vector<double>& row, Emit emit) {
  std::vector<uint8_t>& bytes = f.bytes;
  const std::vector<Elem>& elems = f.elems;
  const Elem& V = f.vertex();
  const int vi = f.vi;
  row.assign(V.props.size(), 0.0);
  if (f.ascii) {
    // strtod / strtol stop at the terminating NUL, never past the buffer
    bytes.push_back('\0');
    const char* p = (const char*)bytes.data() + f.hdr_end;
    const char* end = (const char*)bytes.data() + bytes.size() - 1;
    auto next_line = [&]() {
      while (p < end && *p != '\n') ++p;
      if (p < end) ++p;
    };
    for (int e = 0; e < vi; ++e)
      for (uint64_t r = 0; r < elems[e].count && p < end; ++r) next_line();
    for (uint64_t i = 0; i < V.count; ++i) {
      if (p >= end) return PTGS_EIO;  // fewer rows than the header's vertex count
      for (size_t k = 0; k < V.props.size(); ++k) {
        char* q = nullptr;
        if (V.props[k].list) {  // count then items
          long cnt = strtol(p, &q, 10);
          if (q == p || cnt < 0) return PTGS_EIO;
          p = q;
          for (long t = 0; t < cnt; ++t) { strtod(p, &q); if (q == p) return PTGS_EIO; p = q; }
          row[k] = 0;
          continue;
        }
        row[k] = strtod(p, &q);
        if (q == p) return PTGS_EIO;
        p = q;
      }
      emit(i);
      next_line();
    }
    return PTGS_OK;
  }
  const size_t off = f.vert_off, rs = f.vert_rs;
  for (uint64_t i = 0; i < V.count; ++i) {
    const uint8_t* q = bytes.data() + off + i * rs;
    for (size_t k = 0; k < V.props.size(); ++k) {
      row[k] = read_bin(q, V.props[k].type, f.big);
      q += V.props[k].size;
    }
    emit(i);
  }
  return PTGS_OK;
}

}  // namespace

extern "C" int ptgs_read_ply(const char* path, float* xyz, float* normals, uint8_t* rgb, uint32_t capacity,
                             uint32_t* count) {
  if (!path || !count) return PTGS_EINVAL;
  PlyFile f;
  if (int rc = ply_open(path, f)) return rc;
  const Elem& V = f.vertex();
  *count = (uint32_t)V.count;
  if (!xyz && !normals && !rgb) return PTGS_OK;
  if (capacity < V.count) return PTGS_ERANGE;
  int ix[3] = {-1, -1, -1}, in[3] = {-1, -1, -1}, ic[3] = {-1, -1, -1}, idc[3] = {-1, -1, -1};
  const char* names[4][3] = {{"x", "y", "z"}, {"nx", "ny", "nz"}, {"red", "green", "blue"}, {"f_dc_0", "f_dc_1", "f_dc_2"}};
  int* slots[4] = {ix, in, ic, idc};
  for (size_t p = 0; p < V.props.size(); ++p)
    for (int g = 0; g < 4; ++g)
      for (int a = 0; a < 3; ++a)
        if (V.props[p].name == names[g][a] && !V.props[p].list) slots[g][a] = (int)p;
  if (ix[0] < 0 || ix[1] < 0 || ix[2] < 0) return PTGS_EIO;
  const bool have_n = in[0] >= 0 && in[1] >= 0 && in[2] >= 0;
  const bool have_c = ic[0] >= 0 && ic[1] >= 0 && ic[2] >= 0;
  const bool have_dc = idc[0] >= 0 && idc[1] >= 0 && idc[2] >= 0;
  std::vector<double> row;
  return ply_vertex_rows(f, row, [&](uint64_t i) {
    for (int a = 0; a < 3; ++a) {
      if (xyz) xyz[3 * i + a] = (float)row[ix[a]];
      if (normals) normals[3 * i + a] = have_n ? (float)row[in[a]] : 0.0f;
      if (rgb) {
        uint8_t c = 0;
        if (have_c) c = to_u8(row[ic[a]], is_float_type(V.props[ic[a]].type));
        else if (have_dc) c = to_u8(0.5 + 0.28209479177387814 * row[idc[a]], true);
        rgb[3 * i + a] = c;
      }
    }
  });
}

// Trained-3DGS checkpoint: see ptgs_host.h. The properties are found by name; f_rest_j must be numbered
// 0 .. n-1 without a gap, n = 3 ((d+1)^2 - 1) for a degree d in 0..3.
extern "C" int ptgs_read_gaussian_ply(const char* path, float* means, float* log_scales, float* rotations,
                                      float* opacity_logits, float* sh, uint32_t capacity, uint32_t* count,
                                      uint32_t* sh_degree) {
  if (!path || !count || !sh_degree) return PTGS_EINVAL;
  PlyFile f;
  if (int rc = ply_open(path, f)) return rc;
  const Elem& V = f.vertex();
  int ix[3] = {-1, -1, -1}, idc[3] = {-1, -1, -1}, isc[3] = {-1, -1, -1}, irot[4] = {-1, -1, -1, -1}, iop = -1;
  int irest[45];
  std::fill(irest, irest + 45, -1);
  int n_rest = 0;  // f_rest_* properties, whatever their numbers
  auto indexed = [](const std::string& name, const char* prefix, int limit) {  // "<prefix><j>", j < limit, else -1
    const size_t n = strlen(prefix);
    if (name.compare(0, n, prefix) != 0 || name.size() == n || name.size() > n + 2) return -1;
    int j = 0;
    for (size_t k = n; k < name.size(); ++k) {
      if (name[k] < '0' || name[k] > '9') return -1;
      j = j * 10 + (name[k] - '0');
    }
    if (name.size() == n + 2 && name[n] == '0') return -1;  // "f_rest_07" is not f_rest_7
    return j < limit ? j : -1;
  };
  for (size_t p = 0; p < V.props.size(); ++p) {
    const Prop& pr = V.props[p];
    if (pr.list) continue;
    const std::string& nm = pr.name;
    int j;
    if (nm == "x" || nm == "y" || nm == "z") ix[nm[0] - 'x'] = (int)p;
    else if (nm == "opacity") iop = (int)p;
    else if ((j = indexed(nm, "f_dc_", 3)) >= 0) idc[j] = (int)p;
    else if ((j = indexed(nm, "scale_", 3)) >= 0) isc[j] = (int)p;
    else if ((j = indexed(nm, "rot_", 4)) >= 0) irot[j] = (int)p;
    else if (nm.compare(0, 7, "f_rest_") == 0) {
      ++n_rest;
      if ((j = indexed(nm, "f_rest_", 45)) >= 0) irest[j] = (int)p;
    }
  }
  for (int a = 0; a < 3; ++a)
    if (ix[a] < 0 || idc[a] < 0 || isc[a] < 0) return PTGS_EIO;
  for (int a = 0; a < 4; ++a)
    if (irot[a] < 0) return PTGS_EIO;
  if (iop < 0) return PTGS_EIO;
  int deg = -1;
  for (int d = 0; d <= 3; ++d)
    if (n_rest == 3 * ((d + 1) * (d + 1) - 1)) deg = d;
  if (deg < 0) return PTGS_EIO;
  for (int j = 0; j < n_rest; ++j)
    if (irest[j] < 0) return PTGS_EIO;  // a gap in the numbering (or a number twice)
  *count = (uint32_t)V.count;
  *sh_degree = (uint32_t)deg;
  if (!means && !log_scales && !rotations && !opacity_logits && !sh) return PTGS_OK;
  if (capacity < V.count) return PTGS_ERANGE;
  const size_t K = (size_t)(deg + 1) * (deg + 1);
  std::vector<double> row;
  return ply_vertex_rows(f, row, [&](uint64_t i) {
    for (int a = 0; a < 3; ++a) {
      if (means) means[3 * i + a] = (float)row[ix[a]];
      if (log_scales) log_scales[3 * i + a] = (float)row[isc[a]];
    }
    for (int a = 0; a < 4; ++a)
      if (rotations) rotations[4 * i + a] = (float)row[irot[a]];
    if (opacity_logits) opacity_logits[i] = (float)row[iop];
    if (sh) {
      float* o = sh + i * K * 3;
      for (int c = 0; c < 3; ++c) {
        o[c] = (float)row[idc[c]];
        for (size_t k = 1; k < K; ++k) o[k * 3 + c] = (float)row[irest[c * (K - 1) + (k - 1)]];
      }
    }
  });
}

// The writer of such a checkpoint: see ptgs_host.h. A Gaussian's row is 14 + 3 (d+1)^2 floats, written through one
// buffer per 4096 rows; every float goes out as its four bytes, least significant first.
extern "C" int ptgs_write_gaussian_ply(const char* path, const float* means, const float* log_scales,
                                       const float* rotations, const float* opacity_logits, const float* sh,
                                       uint32_t count, uint32_t sh_degree) {
  if (!path || sh_degree > 3) return PTGS_EINVAL;
  if (count && (!means || !log_scales || !rotations || !opacity_logits || !sh)) return PTGS_EINVAL;
  const size_t K = (size_t)(sh_degree + 1) * (sh_degree + 1), n_rest = 3 * (K - 1);
  std::string hdr = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(count) + "\n";
  auto prop = [&](const std::string& name) { hdr += "property float " + name + "\n"; };
  for (const char* nm : {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"}) prop(nm);
  for (size_t j = 0; j < n_rest; ++j) prop("f_rest_" + std::to_string(j));
  prop("opacity");
  for (int a = 0; a < 3; ++a) prop("scale_" + std::to_string(a));
  for (int a = 0; a < 4; ++a) prop("rot_" + std::to_string(a));
  hdr += "end_header\n";
  FILE* f = std::fopen(path, "wb");
  if (!f) return PTGS_EIO;
  bool ok = std::fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size();
  const size_t row_floats = 14 + 3 * K, chunk = 4096;
  std::vector<uint8_t> buf;
  buf.reserve(chunk * row_floats * 4);
  auto put = [&](float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    for (int b = 0; b < 4; ++b) buf.push_back((uint8_t)(u >> (8 * b)));
  };
  for (size_t i0 = 0; i0 < count && ok; i0 += chunk) {
    buf.clear();
    const size_t i1 = std::min<size_t>(count, i0 + chunk);
    for (size_t i = i0; i < i1; ++i) {
      const float* s = sh + i * K * 3;
      for (int a = 0; a < 3; ++a) put(means[3 * i + a]);
      for (int a = 0; a < 3; ++a) put(0.0f);  // nx ny nz
      for (int c = 0; c < 3; ++c) put(s[c]);
      for (int c = 0; c < 3; ++c)  // f_rest is channel-major: f_rest[c (K - 1) + (k - 1)] = sh[i][k][c]
        for (size_t k = 1; k < K; ++k) put(s[k * 3 + c]);
      put(opacity_logits[i]);
      for (int a = 0; a < 3; ++a) put(log_scales[3 * i + a]);
      for (int a = 0; a < 4; ++a) put(rotations[4 * i + a]);
    }
    ok = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  }
  return (std::fclose(f) == 0 && ok) ? PTGS_OK : PTGS_EIO;
}
