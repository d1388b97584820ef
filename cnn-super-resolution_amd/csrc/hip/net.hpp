// net.hpp -- the nets of the fused families as types, and the dispatch from a
// srcnn_net to the instantiated one.  Included, inside namespace srcnn::fused,
// by the two plan headers: fused_plan.hpp (train_fused.hip) and fwd_plan.hpp
// (forward_fused.hip), one of them per unit; each names its own list of nets.
// Host code without any HIP call.

template <int N1_, int N2_, int F1_, int F3_>
struct Net {
  static constexpr int N1 = N1_, N2 = N2_, F1 = F1_, F3 = F3_;
  static constexpr int P12 = F1 * F1 * N1 + N1 + N1 * N2 + N2;
  static constexpr int P3 = F3 * F3 * N2 + 1;
  // layers 1-2 of the default net: the split-bf16 pair and d1c are built for them
  static constexpr bool kDefault12 = N1 == 64 && N2 == 32 && F1 == 9;
  // the default net: fwd_l123x6 is built for it
  static constexpr bool kDefault = kDefault12 && F3 == 5;
};

// The instantiated nets, once: f(Net<..>{}) of the one that `net` is, else 0.
// plan, run and preload all dispatch through here.
template <typename F, typename... Ns>
static int first_net(const srcnn_net* net, F&& f, Ns... ns) {
  int rc = 0;
  auto is = [&](auto n) {
    return net->n1 == (uint32_t)n.N1 && net->n2 == (uint32_t)n.N2 && net->f1 == (uint32_t)n.F1 &&
           net->f2 == 1 && net->f3 == (uint32_t)n.F3;
  };
  (void)((is(ns) && (rc = f(ns), true)) || ...);
  return rc;
}
