// TEST HARNESS (not product): one forward pass (plg::Forward) of the host instantiation of the lane-group planar step
// with the solver's iteration cap chosen by the caller, the lanes' qacc, Ma and gradient handed back raw.  Built on
// planar_lg_host.cpp (HostCx, planar_lg_step); used by tests/test_planar_lg_first_trip_host.py.
#include "planar_lg_host.cpp"

// `passes` forward passes at the same (q, v, ctrl), qacc_warmstart carried from one to the next (the second pass of
// two starts at the first one's result); out_* [kLV][KL] and iters [KL] are the last pass's
template <int KL>
static void RunForward(int model, const double* q, const double* v, const double* warm, const double* ctrl,
                       int max_iter, int passes, double* out_qacc, double* out_ma, double* out_grad, int* iters) {
  using V = plg::LV<double, KL>;
  using G = plg::Grp<KL>;
  const CheetahModel<double> m = model == 0 ? BuildCheetahModel()
                                 : model == 3 ? BuildHopperModel() : BuildWalkerModel(model == 2);
  const int pm = model == 0 ? kPlanarCheetah : (model == 3 ? kPlanarHopper : kPlanarWalker);
  double tab[plg::Tab<KL>::kSize];
  plg::BuildTable<KL>(m, tab);
  HostCx<KL> cx;
  cx.tab = tab;
  const plg::SolverCfgLg<double> cfg{max_iter, 1e-13};
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
  V qacc[plg::kLV], Ma[plg::kLV], grad[plg::kLV], it = V(0);
  for (int pass = 0; pass < passes; ++pass) {
    plg::Pos<V> p;
    it = plg::Forward<KL>(m, cfg, cx, lq, lv, lw, lc, p, qacc, Ma, grad);
  }
  for (int c = 0; c < KL; ++c) {
    for (int i = 0; i < plg::kLV; ++i) {
      out_qacc[i * KL + c] = qacc[i].v[c];
      out_ma[i * KL + c] = Ma[i].v[c];
      out_grad[i * KL + c] = grad[i].v[c];
    }
    iters[c] = (int)it.v[c];
  }
}

extern "C" void planar_lg_forward(int model, int kl, const double* q, const double* v, const double* warm,
                                  const double* ctrl, int max_iter, int passes, double* out_qacc, double* out_ma,
                                  double* out_grad, int* iters) {
  if (kl == 1) return RunForward<1>(model, q, v, warm, ctrl, max_iter, passes, out_qacc, out_ma, out_grad, iters);
  if (kl == 2) return RunForward<2>(model, q, v, warm, ctrl, max_iter, passes, out_qacc, out_ma, out_grad, iters);
  RunForward<4>(model, q, v, warm, ctrl, max_iter, passes, out_qacc, out_ma, out_grad, iters);
}
