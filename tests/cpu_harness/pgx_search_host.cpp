// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_search.hip.h, built with g++ by
// tests/test_pgx_search_host.py.  It runs the search the way the kernel's wave does -- lane j owns actions j and
// j + 64, scores and reductions go lane by lane -- with the wave's lanes walked as loops.  Positions come in as the
// hidden words of pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by envpool_amd/.
#include <cstdint>
#include <vector>

#include "../../envpool_amd/csrc/pgx_search.hip.h"

using namespace epa::pgx;

namespace {
template <int G>
int Run(int n, const int32_t* hidden, const uint8_t* done, const int32_t* env_ids, int simulations, int leaf_playouts,
        float c_puct, int max_plies, uint64_t seed, int32_t* visits, int32_t* returns, int32_t* action,
        int32_t* nodes_used) {
  constexpr int W = HiddenWords<G>(), A = Dims<G>::A, L = kSearchWave, SL = SearchSlotsPerLane<G>();
  const int limit = PlayoutLimit(max_plies);
  std::vector<SearchNode<G>> nodes((size_t)simulations + 1);
  std::vector<int> path_node(kSearchMaxPath), path_act(kSearchMaxPath);
  for (int i = 0; i < n; ++i) {
    int32_t* vis = visits + (size_t)i * A;
    int32_t* ret = returns + (size_t)i * A;
    for (int a = 0; a < A; ++a) vis[a] = ret[a] = 0;
    action[i] = -1;
    nodes_used[i] = 0;
    State root{};
    if (!SetHidden<G>(root, hidden + (size_t)i * W)) return -2;
    root.done = done[i] ? 1 : 0;
    if (done[i]) continue;
    nodes[0].s = root;
    nodes[0].term0 = 0;
    for (int lane = 0; lane < L; ++lane) {
      for (int j = 0; j < SL; ++j) {
        if (lane + L * j < A) SearchClearEdge<G>(nodes[0], lane + L * j);
      }
    }
    int count = 1;
    for (int t = 0; t < simulations; ++t) {
      int node = 0, depth = 0, val0 = 0;
      for (;;) {
        SearchNode<G>& nd = nodes[(size_t)node];
        if (nd.s.done) {
          val0 = leaf_playouts * nd.term0;
          break;
        }
        int total = 0;  // the wave sum of the lanes' own visits
        for (int lane = 0; lane < L; ++lane) {
          for (int j = 0; j < SL; ++j) {
            if (lane + L * j < A) total += nd.v[lane + L * j];
          }
        }
        const int sign = SearchSign<G>(nd.s);
        SearchPick best = SearchNone();
        for (int lane = L - 1; lane >= 0; --lane) {  // (any order: SearchBetter is associative and commutative)
          SearchPick mine = SearchNone();
          for (int j = 0; j < SL; ++j) {
            const int a = lane + L * j;
            if (a < A && Has(nd.s.m, a)) {
              mine = SearchBetter(
                  mine, SearchPick{SearchScore(nd.v[a], nd.w0[a], total, sign, leaf_playouts, c_puct), a, 1});
            }
          }
          best = SearchBetter(best, mine);
        }
        const int a = best.action;
        if (a < 0 || depth >= kSearchMaxPath) return -3;  // a running game has a legal action; paths are short
        path_node[(size_t)depth] = node;
        path_act[(size_t)depth] = a;
        ++depth;
        if (nd.child[a] < 0) {
          SearchNode<G>& c = nodes[(size_t)count];
          c.term0 = SearchExpand<G>(nd.s, a, c.s);
          for (int lane = 0; lane < L; ++lane) {
            for (int j = 0; j < SL; ++j) {
              if (lane + L * j < A) SearchClearEdge<G>(c, lane + L * j);
            }
          }
          nd.child[a] = count++;
          if (c.s.done) {
            val0 = leaf_playouts * c.term0;
          } else {
            for (int lane = 0; lane < L; ++lane) {
              if (lane < leaf_playouts) val0 += SearchLeaf<G>(c.s, seed, env_ids[i], t, leaf_playouts, lane, limit);
            }
          }
          break;
        }
        node = nd.child[a];
      }
      for (int d = 0; d < depth; ++d) {
        SearchNode<G>& nd = nodes[(size_t)path_node[(size_t)d]];
        nd.v[path_act[(size_t)d]] += 1;
        nd.w0[path_act[(size_t)d]] += val0;
      }
    }
    const int sign = SearchSign<G>(root);
    SearchPick best = SearchNone();
    for (int a = 0; a < A; ++a) {
      vis[a] = nodes[0].v[a];
      ret[a] = sign * nodes[0].w0[a];
      if (Has(root.m, a)) best = SearchBetter(best, SearchPick{(float)vis[a], a, 1});
    }
    action[i] = best.action;
    nodes_used[i] = count;
  }
  return 0;
}
}  // namespace

extern "C" {

// n roots (hidden[i]: HiddenWords words, done[i]) with global ids env_ids[i].  Row i of visits / returns [n, A] and
// action [n]: the results of the contract; nodes_used [n]: the nodes of the root's tree.  -1: no such game; -2: words
// that are no position; -3: a broken invariant.
int pgx_search(int game, int n, const int32_t* hidden, const uint8_t* done, const int32_t* env_ids, int simulations,
               int leaf_playouts, float c_puct, int max_plies, uint64_t seed, int32_t* visits, int32_t* returns,
               int32_t* action, int32_t* nodes_used) {
  switch (game) {
    case kTicTacToe:
      return Run<kTicTacToe>(n, hidden, done, env_ids, simulations, leaf_playouts, c_puct, max_plies, seed, visits,
                             returns, action, nodes_used);
    case kConnectFour:
      return Run<kConnectFour>(n, hidden, done, env_ids, simulations, leaf_playouts, c_puct, max_plies, seed, visits,
                               returns, action, nodes_used);
    case kHex:
      return Run<kHex>(n, hidden, done, env_ids, simulations, leaf_playouts, c_puct, max_plies, seed, visits, returns,
                       action, nodes_used);
    case kOthello:
      return Run<kOthello>(n, hidden, done, env_ids, simulations, leaf_playouts, c_puct, max_plies, seed, visits,
                           returns, action, nodes_used);
    default: return -1;
  }
}

int pgx_search_node_bytes(int game) {
  switch (game) {
    case kTicTacToe: return (int)sizeof(SearchNode<kTicTacToe>);
    case kConnectFour: return (int)sizeof(SearchNode<kConnectFour>);
    case kHex: return (int)sizeof(SearchNode<kHex>);
    case kOthello: return (int)sizeof(SearchNode<kOthello>);
    default: return -1;
  }
}

}  // extern "C"
