// The argument checks and small helpers the host staging files share (resident.cpp, tsne.cpp, umap.cpp, kmeans.cpp, louvain.cpp).
// `w` is the entry point's name as its messages carry it.  The order in which an entry point calls these is part of the ABI's
// behaviour and stays with the entry point.
#pragma once
#include <cmath>
#include <cstdio>

#include "engine.h"

namespace sapca {
namespace resident {

inline std::string num(uint64_t v) { return std::to_string(v); }
inline std::string numd(double v) {
  char buf[40];
  std::snprintf(buf, sizeof(buf), "%g", v);
  return buf;
}

inline void check_constant(double v, const char* name, const std::string& w) {
  SAPCA_CHECK(std::isfinite(v) && v >= 0.0, SAPCA_ERR_ARG, w + ": " + name + " = " + numd(v) + " must be finite and not negative");
}

inline void check_rows(uint64_t m, const std::string& w) {
  SAPCA_CHECK(m < (1ull << 31), SAPCA_ERR_ARG, w + ": m = " + num(m) + " rows; 2^31 or more are not supported");
}

// the limits of the neighbour search (knn.hip) on a panel's width and on the row stride called `ldname`
inline void check_panel_width(uint64_t d, const std::string& w) {
  SAPCA_CHECK(d != 0, SAPCA_ERR_ARG, w + ": d is 0");
  SAPCA_CHECK(d <= 1024, SAPCA_ERR_ARG, w + ": d = " + num(d) + " exceeds 1024 columns");
}
inline void check_stride_covers(uint64_t d, uint64_t ld, const char* ldname, const std::string& w) {
  SAPCA_CHECK(ld >= d, SAPCA_ERR_ARG, w + ": " + ldname + " = " + num(ld) + " is less than d = " + num(d));
}
inline void check_stride_limit(uint64_t ld, const std::string& w) {
  SAPCA_CHECK(ld < (1ull << 28), SAPCA_ERR_ARG, w + ": a row stride of " + num(ld) + " elements; 2^28 or more are not supported");
}
inline void check_panel(uint64_t d, uint64_t ld, const char* ldname, const std::string& w) {
  check_panel_width(d, w);
  check_stride_covers(d, ld, ldname, w);
  check_stride_limit(ld, w);
}

// the header of a versioned struct `arg` of the ABI (`name`: its type as the message names it); options may not be null
template <typename S>
void check_struct_size(const S* o, const char* arg, const char* name, const std::string& w) {
  SAPCA_CHECK(o->struct_size == sizeof(S), SAPCA_ERR_ARG,
              w + ": " + arg + "->struct_size is " + num(o->struct_size) + ", this library's " + name + " has " + num(sizeof(S)) + " bytes");
}
template <typename S>
void check_options_header(const S* o, const char* name, const std::string& w) {
  SAPCA_CHECK(o != nullptr, SAPCA_ERR_ARG, w + ": null options");
  check_struct_size(o, "options", name, w);
}

inline int cu_count(sapca_handle_s& h) {
  int n = 0;
  SAPCA_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, h.device));
  return n;
}

// The host routes: x (nx elements) up into bx, y (ny elements) up into by where it is an input, run(dx, dy) -- the device route
// -- and y down again.  More results of run() may be queued behind it: the caller synchronises.
template <typename T, typename Run>
void host_route(sapca_handle_s& h, DevBuf& bx, const T* x, size_t nx, DevBuf& by, T* y, size_t ny, bool y_given, Run&& run) {
  hipStream_t s = h.stream;
  T* dx = bx.as<T>(nx);
  T* dy = by.as<T>(ny);
  SAPCA_HIP(hipMemcpyAsync(dx, x, nx * sizeof(T), hipMemcpyHostToDevice, s));
  if (y_given) SAPCA_HIP(hipMemcpyAsync(dy, y, ny * sizeof(T), hipMemcpyHostToDevice, s));
  run(dx, dy);
  SAPCA_HIP(hipMemcpyAsync(y, dy, ny * sizeof(T), hipMemcpyDeviceToHost, s));
}

}  // namespace resident
}  // namespace sapca
