// The affine map of the chunked RTS pass: ms_in = G ms_out + g, the smoothed
// mean entering a run of steps as a function of the mean leaving it.  Stored
// as R*R + R doubles, [G (row-major) | g].
//
// Every sum below is an explicit fma chain in ascending k, started from 0 for
// a matrix product and from the offset for a mean: a map composed or applied
// by any kernel has the same bits, whichever unit does it.
#pragma once
#include "handoff.hpp"
#include "small_linalg.hpp"

namespace eks {

template <int R>
struct Affine {
  static constexpr int len = R * R + R;
  double G[R][R], g[R];
  EKS_DEV void set_identity() {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      g[i] = 0.0;
#pragma unroll
      for (int j = 0; j < R; ++j) G[i][j] = (i == j) ? 1.0 : 0.0;
    }
  }
  // the stored layout: get(k) reads / put(k, v) writes element k of the map
  template <typename Get>
  EKS_DEV void load_at(Get &&get) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      g[i] = get(R * R + i);
#pragma unroll
      for (int j = 0; j < R; ++j) G[i][j] = get(i * R + j);
    }
  }
  template <typename Put>
  EKS_DEV void store_at(Put &&put) const {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      put(R * R + i, g[i]);
#pragma unroll
      for (int j = 0; j < R; ++j) put(i * R + j, G[i][j]);
    }
  }
  // a row in global memory or LDS
  EKS_DEV void load(const double *row) {
    load_at([&](int k) { return row[k]; });
  }
  EKS_DEV void store(double *row) const {
    store_at([&](int k, double v) { row[k] = v; });
  }
  // a row another block publishes / reads (write-through, L1-bypassing)
  EKS_DEV void load_wt(const double *row) {
    load_at([&](int k) { return ld_wt(row + k); });
  }
  EKS_DEV void store_wt(double *row) const {
    store_at([&](int k, double v) { st_wt(row + k, v); });
  }
  static EKS_DEV Affine from(const double *row) {
    Affine f;
    f.load(row);
    return f;
  }
  // ms <- G ms + g (the one expression every application of a map uses, so
  // that a mean carried through any number of maps has the same bits
  // whichever unit applies them)
  EKS_DEV void apply(double (&ms)[R]) const {
    double nx[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      double sm = g[u];
#pragma unroll
      for (int q = 0; q < R; ++q) sm = fma(G[u][q], ms[q], sm);
      nx[u] = sm;
    }
#pragma unroll
    for (int u = 0; u < R; ++u) ms[u] = nx[u];
  }
  // (this o h)(x) = G (Gh x + gh) + g
  EKS_DEV Affine after(const Affine &h) const {
    Affine o;
    matmul<R, R, R>(G, h.G, o.G);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double t = g[i];
#pragma unroll
      for (int k = 0; k < R; ++k) t = fma(G[i][k], h.g[k], t);
      o.g[i] = t;
    }
    return o;
  }
  // after(), one row of G and g at a time: the same sums, issued in the order
  // k3_bwd (two_pass.hpp) was tuned with; its register allocation, at the
  // limit, moves with the order
  EKS_DEV Affine after_by_rows(const Affine &h) const {
    Affine o;
#pragma unroll
    for (int u = 0; u < R; ++u) {
#pragma unroll
      for (int v = 0; v < R; ++v) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < R; ++q) t = fma(G[u][q], h.G[q][v], t);
        o.G[u][v] = t;
      }
      double t = g[u];
#pragma unroll
      for (int q = 0; q < R; ++q) t = fma(G[u][q], h.g[q], t);
      o.g[u] = t;
    }
    return o;
  }
  // this <- this o (J, d), one RTS step absorbed on the right: g with the
  // old G, then G <- G J
  EKS_DEV void then(const double (&J)[R][R], const double (&d)[R]) {
    double GJ[R][R];
    matmul<R, R, R>(G, J, GJ);
    add_image(d);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) G[i][j] = GJ[i][j];
  }
  // the trajectory's last step, ms[T-1] = m: the map ends in a constant
  EKS_DEV void then_const(const double (&m)[R]) {
    add_image(m);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) G[i][j] = 0.0;
  }
  EKS_DEV Affine shfl_down(int delta) const {
    Affine o;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      o.g[i] = __shfl_down(g[i], delta, 64);
#pragma unroll
      for (int j = 0; j < R; ++j) o.G[i][j] = __shfl_down(G[i][j], delta, 64);
    }
    return o;
  }

  // g <- g + G x
  EKS_DEV void add_image(const double (&x)[R]) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double sg = g[i];
#pragma unroll
      for (int u = 0; u < R; ++u) sg = fma(G[i][u], x[u], sg);
      g[i] = sg;
    }
  }
};

}  // namespace eks
