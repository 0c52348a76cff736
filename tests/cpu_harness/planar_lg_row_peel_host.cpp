// TEST HARNESS (not product): one forward pass (plg::Forward) of the host instantiation of the lane-group planar step
// at a state of the caller's, with what the pass over the constraint rows (plg::RowsPass) left per Newton trip handed
// back: the lanes' own slot sets, their active-row masks and their parts of the Hessian.  Built on planar_lg_host.cpp
// (HostCx); used by tests/test_planar_lg_row_peel_host.py.
#include <cstring>

constexpr int kRecTrips = 16, kRecLanes = 4, kRecTri = 21;
static unsigned g_own[kRecLanes];
static unsigned g_mask[kRecTrips][kRecLanes];
static double g_h[kRecTrips][kRecTri][kRecLanes];
static int g_trips;
template <typename U>
static void RecOwn(const U& own) {
  for (unsigned c = 0; c < sizeof(own.v) / sizeof(own.v[0]); ++c) g_own[c] = own.v[c];
}
template <typename U, typename V>
static void RecRows(const U& mask, const V* H) {
  if (g_trips < kRecTrips) {
    for (unsigned c = 0; c < sizeof(mask.v) / sizeof(mask.v[0]); ++c) {
      g_mask[g_trips][c] = mask.v[c];
      for (int k = 0; k < kRecTri; ++k) g_h[g_trips][k][c] = H[k].v[c];
    }
  }
  ++g_trips;
}
#define EPA_LG_HOST_OWN(own) RecOwn(own)
#define EPA_LG_HOST_MASK(mask, H) RecRows(mask, H)

#include "planar_lg_host.cpp"

template <int KL>
static void RunRows(int model, const double* q, const double* v, const double* warm, const double* ctrl,
                    double* out_qacc, double* out_grad, int* iters) {
  using V = plg::LV<double, KL>;
  using G = plg::Grp<KL>;
  const CheetahModel<double> m = model == 0 ? BuildCheetahModel()
                                 : model == 3 ? BuildHopperModel() : BuildWalkerModel(model == 2);
  const int pm = model == 0 ? kPlanarCheetah : (model == 3 ? kPlanarHopper : kPlanarWalker);
  double tab[plg::Tab<KL>::kSize];
  plg::BuildTable<KL>(m, tab);
  HostCx<KL> cx;
  cx.tab = tab;
  const plg::SolverCfgLg<double> cfg{50, 1e-13};
  V lq[plg::kLV], lv[plg::kLV], lw[plg::kLV], lc[3];
  for (int c = 0; c < KL; ++c) {
    const int leg = G::Leg(c);
    for (int i = 0; i < plg::kLV; ++i) {
      const int g = i < 3 ? i : 3 + 3 * leg + (i - 3);
      const int sg = PlanarDofSign(pm, g);
      lq[i].v[c] = sg * q[g];
      lv[i].v[c] = sg * v[g];
      lw[i].v[c] = sg * warm[g];
    }
    lq[0].v[c] = 0;  // local x
    for (int k = 0; k < 3; ++k) {
      const double a = ctrl[3 * leg + k];
      lc[k].v[c] = a < -1 ? -1 : (a > 1 ? 1 : a);
    }
  }
  V qacc[plg::kLV], Ma[plg::kLV], grad[plg::kLV];
  plg::Pos<V> p;
  const V it = plg::Forward<KL>(m, cfg, cx, lq, lv, lw, lc, p, qacc, Ma, grad);
  for (int c = 0; c < KL; ++c) {
    for (int i = 0; i < plg::kLV; ++i) {
      out_qacc[i * KL + c] = qacc[i].v[c];
      out_grad[i * KL + c] = grad[i].v[c];
    }
    iters[c] = (int)it.v[c];
  }
}

// out_qacc, out_grad [kLV][kl]; iters, own [kl]; *trips = passes over the rows the forward pass ran (recorded: the
// first 16); masks [16][kl]; h [16][21][kl]
extern "C" void planar_lg_rows(int model, int kl, const double* q, const double* v, const double* warm,
                               const double* ctrl, double* out_qacc, double* out_grad, int* iters, unsigned* own,
                               int* trips, unsigned* masks, double* h) {
  g_trips = 0;
  std::memset(g_own, 0, sizeof(g_own));
  std::memset(g_mask, 0, sizeof(g_mask));
  std::memset(g_h, 0, sizeof(g_h));
  if (kl == 1) {
    RunRows<1>(model, q, v, warm, ctrl, out_qacc, out_grad, iters);
  } else if (kl == 2) {
    RunRows<2>(model, q, v, warm, ctrl, out_qacc, out_grad, iters);
  } else {
    RunRows<4>(model, q, v, warm, ctrl, out_qacc, out_grad, iters);
  }
  *trips = g_trips;
  for (int c = 0; c < kl; ++c) own[c] = g_own[c];
  for (int t = 0; t < kRecTrips; ++t) {
    for (int c = 0; c < kl; ++c) {
      masks[t * kl + c] = g_mask[t][c];
      for (int k = 0; k < kRecTri; ++k) h[(t * kRecTri + k) * kl + c] = g_h[t][k][c];
    }
  }
}
