// TEST HARNESS (not product): host instantiation of the proven values of envpool_amd/csrc/pgx_guided.hip.h ("Proven
// values"), built with g++ by tests/test_pgx_prove_host.py.  The session is the tactics harness's
// (pgx_tactics_host.cpp, included here; width 1 is the plain session, call for call) begun with a flags word.  With
// kGuidedProve the advance is walked the way the PROVE kernels' wave walks it -- the answers with the climb behind
// every status-1 slot's backup, rule 2 lane by lane over the actions a lane owns and then merged over the lanes, the picks
// that skip proven losses, no descent from a proven root, then the tactics stage -- and result, reroot and the proof
// read-out follow the header's rules 6, 8 and 7.  Without the flag every call is the tactics harness's.  With
// -DPGX_PROVE_MAIN it is a program: three rounds of a ConnectFour and an Othello session with reroots between them.
// Not linked by envpool_amd/.
#include "pgx_tactics_host.cpp"

namespace {
struct ProveSession {
  virtual ~ProveSession() {}
  virtual void Proof(int8_t* value, int8_t* q) const = 0;
};

template <int G>
struct ProveRun : TacticsRun<G>, ProveSession {
  using Base = TacticsRun<G>;
  static constexpr int A = Dims<G>::A, L = kSearchWave, SL = SearchSlotsPerLane<G>();
  int flags;

  ProveRun(int n_, int s, int cap, int w, float c, int d, long long m, int f)
      : Base(n_, s, cap, w, c, d, m), flags(f) {}

  // rule 2 at node `nd` of `tree`: every lane over the actions it owns, then the lanes merged.  cv (may be null): [A],
  // the children's proven values for nd's mover
  int Rule2(const GuidedNode<G>* tree, const GuidedNode<G>& nd, int* cv) const {
    const int sign = SearchSign<G>(nd.s);
    GuidedProofAcc wave = GuidedProofNone();
    for (int lane = 0; lane < L; ++lane) {
      GuidedProofAcc acc = GuidedProofNone();
      for (int q = 0; q < SL; ++q) {
        const int a = lane + L * q;
        if (a >= A) continue;
        int c = kGuidedUnproven;
        if (Has(nd.s.m, a)) {
          const int ch = nd.child[a];
          if (ch >= 0 && ch < this->capacity) c = GuidedProofOf(tree[ch].s.done, tree[ch].term0, sign);
          acc = GuidedProofAdd(acc, c);
        }
        if (cv != nullptr) cv[a] = c;
      }
      wave = GuidedProofMerge(wave, acc);
    }
    return GuidedProofValue(wave);
  }

  // rule 3: GuidedClimb of pgx.hip
  int Climb(GuidedNode<G>* tree, const int32_t* path, int depth, int pending) const {
    int below = pending;
    for (int d = depth - 1; d >= 0; --d) {
      if (tree[below].s.done == 0) break;
      const int nidx = path[d] >> 8;
      GuidedNode<G>& nd = tree[nidx];
      const int v = Rule2(tree, nd, nullptr);
      if (v == kGuidedUnproven) break;
      if (nidx == 0) return v;
      GuidedTacticsMark<G>(nd, v);
      below = nidx;
    }
    return kGuidedUnproven;
  }

  // PgxGuidedAdvanceWide<.., PROVE> and PgxGuidedTactics, one root after the other
  int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    if ((flags & kGuidedProve) == 0) return Base::Advance(priors, values, obs, mask, status);
    if (this->calls > this->simulations) return -4;
    const int W = this->width;
    int rc = 0;
    std::vector<int> cv((size_t)A);
    for (int i = 0; i < this->n; ++i) {
      GuidedWideRoot& rec = this->Rec(i);
      GuidedWideSlot* slots = GuidedWideSlots(rec);
      GuidedNode<G>* tree = this->Tree(i);
      int done = rec.done;
      int proof = GuidedProofDecode(rec.pad[0]);
      // A. the answers
      for (int j = 0; j < W; ++j) {
        const int st = slots[j].status;
        if (st == kGuidedIdle) continue;
        GuidedNode<G>& leaf = tree[slots[j].pending];
        const size_t lrow = (size_t)i * W + j;
        float val0;
        if (st == kGuidedEvaluate) {
          for (int lane = 0; lane < L; ++lane) {
            for (int q = 0; q < SL; ++q) {
              const int a = lane + L * q;
              if (a < A) leaf.p[a] = GuidedClean(priors[lrow * A + a]);
            }
          }
          val0 = (float)SearchSign<G>(leaf.s) * GuidedCleanV(values[lrow]);
        } else {
          val0 = (float)leaf.term0;
        }
        for (int d = 0; d < slots[j].depth; ++d) {
          GuidedNode<G>& nd = tree[slots[j].path[d] >> 8];
          nd.v[slots[j].path[d] & 255] += 1;
          nd.w0[slots[j].path[d] & 255] += val0;
        }
        if (slots[j].depth > 0) ++done;
        if (st == kGuidedTerminal) {
          const int got = Climb(tree, slots[j].path, slots[j].depth, slots[j].pending);
          if (got != kGuidedUnproven) {
            proof = got;
            rec.pad[0] = GuidedProofEncode(proof);
          }
        }
      }
      // B. the descents: none from a proven root
      int count = rec.count;
      const bool idle = rec.over != 0 || rec.broken != 0 || proof != kGuidedUnproven;
      int my_depth[L], my_pend[L];
      for (int lane = 0; lane < L; ++lane) {
        my_depth[lane] = 0;
        my_pend[lane] = -1;
      }
      int j = 0;
      bool broken = false;
      const State root = tree[0].s;
      for (; j < W && !idle; ++j) {
        if (!(done + j < this->simulations && count < this->capacity)) break;
        int node = 0, depth = 0;
        bool collided = false;
        State s = root;
        for (;;) {
          GuidedNode<G>& nd = tree[node];
          int o[L][SL], own = 0, osum = 0;
          for (int lane = 0; lane < L; ++lane) {
            for (int q = 0; q < SL; ++q) {
              o[lane][q] = 0;
              if (lane + L * q < A) own += nd.v[lane + L * q];
            }
          }
          for (int i2 = 0; i2 < j && i2 < L; ++i2) {
            const int e = depth < my_depth[i2] ? this->lpath[(size_t)depth * W + i2] : -1;
            if (!GuidedWideOn(e, my_depth[i2], depth, node)) continue;
            ++osum;
            const int ai = e & 255;
            o[ai & (L - 1)][ai / L] += 1;
          }
          const int total = own + osum;
          const int sign = SearchSign<G>(s);
          Rule2(tree, nd, cv.data());  // (the pick uses the children's values alone)
          SearchPick open = SearchNone(), all = SearchNone();
          for (int lane = L - 1; lane >= 0; --lane) {
            SearchPick mine = SearchNone(), mine_all = SearchNone();
            for (int q = 0; q < SL; ++q) {
              const int a = lane + L * q;
              if (a < A && Has(s.m, a)) {
                const SearchPick p{GuidedWideScore(nd.v[a], nd.w0[a], nd.p[a], o[lane][q], total, sign, this->c_puct),
                                   a, 1};
                mine_all = SearchBetter(mine_all, p);
                if (!GuidedProofClosed(cv[(size_t)a])) mine = SearchBetter(mine, p);
              }
            }
            open = SearchBetter(open, mine);
            all = SearchBetter(all, mine_all);
          }
          const int a = open.action >= 0 ? open.action : all.action;
          if (a < 0 || depth >= kSearchMaxPath) {
            broken = true;
            break;
          }
          this->lpath[(size_t)depth * W + j] = node << 8 | a;
          slots[j].path[depth] = node << 8 | a;
          ++depth;
          if (nd.child[a] < 0) {
            const int c = count++;
            GuidedNode<G>& nn = tree[c];
            nn.term0 = SearchExpand<G>(s, a, nn.s);
            Run<G>::ClearNode(nn);
            nd.child[a] = c;
            node = c;
            s = nn.s;
            break;
          }
          node = nd.child[a];
          s = tree[node].s;
          if (s.done) break;
          for (int i2 = 0; i2 < j; ++i2) collided = collided || my_pend[i2] == node;
          if (collided) break;
        }
        if (broken || collided) break;
        const int st = s.done ? kGuidedTerminal : kGuidedEvaluate;
        slots[j].pending = node;
        slots[j].status = st;
        slots[j].depth = depth;
        my_depth[j] = depth;
        my_pend[j] = st == kGuidedEvaluate ? node : -1;
        this->Emit(i * W + j, st, s, obs, mask, status);
      }
      if (broken) j = 0;
      for (int q = j; q < W; ++q) {
        slots[q].status = kGuidedIdle;
        slots[q].depth = 0;
        this->Emit(i * W + q, kGuidedIdle, root, obs, mask, status);
      }
      rec.count = count;
      rec.done = done;
      rec.live = j;
      if (broken) {
        rec.broken = 1;
        rc = -3;
      }
    }
    ++this->calls;
    // the tactics stage, unchanged (TacticsRun::Advance behind its own descents)
    if (this->depth == 0) return rc;
    for (int i = 0; i < this->n; ++i) {
      GuidedWideSlot* slots = GuidedWideSlots(this->Rec(i));
      for (int j = 0; j < W; ++j) {
        this->given_up[(size_t)i * W + j] = 0;
        if (!GuidedTacticsLooksAt(slots[j].status, slots[j].pending)) continue;
        GuidedNode<G>& leaf = this->Tree(i)[slots[j].pending];
        const State s = leaf.s;
        const Solved out = SolveOne<G>(s, this->depth, this->max_nodes, *this->top, this->lanes, this->stack);
        this->solved_nodes[(size_t)i] += out.nodes;
        this->given_up[(size_t)i * W + j] = out.status == kSolveGivenUp;
        if (!GuidedTacticsDecides(out.status, out.value)) continue;
        GuidedTacticsMark<G>(leaf, out.value);
        slots[j].status = kGuidedTerminal;
        ++this->decided[(size_t)i];
        this->Emit(i * W + j, kGuidedTerminal, s, obs, mask, status);
      }
    }
    return rc;
  }

  // PgxGuidedResult<.., PROVE>: rule 6 over the plain result
  void Result(int32_t* visits, float* values, int32_t* action, int32_t* nodes_used, int32_t* done) override {
    Base::Result(visits, values, action, nodes_used, done);
    if ((flags & kGuidedProve) == 0) return;
    std::vector<int> cv((size_t)A);
    for (int i = 0; i < this->n; ++i) {
      if (this->Rec(i).over != 0) continue;
      const GuidedNode<G>& n0 = this->Tree(i)[0];
      const int proof = GuidedProofDecode(this->Rec(i).pad[0]);
      Rule2(this->Tree(i), n0, cv.data());
      SearchPick best = SearchNone();
      for (int a = 0; a < A; ++a) {
        if (Has(n0.s.m, a) && GuidedProofPlays(proof, cv[(size_t)a])) {
          best = SearchBetter(best, SearchPick{(float)n0.v[a], a, 1});
        }
      }
      if (best.action >= 0) action[i] = best.action;
    }
  }

  // PgxGuidedReroot<.., PROVE>: rule 8 behind the reroot
  int Reroot(const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    const int rc = Base::Reroot(actions, s2, obs, mask, status);
    if (rc != 0 || (flags & kGuidedProve) == 0) return rc;
    for (int i = 0; i < this->n; ++i) {
      GuidedWideRoot& rec = this->Rec(i);
      int proof = kGuidedUnproven;
      if (rec.over == 0) proof = Rule2(this->Tree(i), this->Tree(i)[0], nullptr);  // (a fresh root has no child)
      rec.pad[0] = GuidedProofEncode(proof);
    }
    return rc;
  }

  // PgxGuidedProof
  void Proof(int8_t* value, int8_t* q) const override {
    std::vector<int> cv((size_t)A);
    for (int i = 0; i < this->n; ++i) {
      const GuidedWideRoot& rec = GuidedWideRootAt(const_cast<char*>(this->roots.data()), i, this->width);
      const GuidedNode<G>* tree = this->nodes.data() + (size_t)i * this->capacity;
      const bool none = (flags & kGuidedProve) == 0 || rec.over != 0;
      if (!none) Rule2(tree, tree[0], cv.data());
      for (int a = 0; a < A; ++a) q[(size_t)i * A + a] = (int8_t)(none ? kGuidedUnproven : cv[(size_t)a]);
      value[i] = (int8_t)(none ? kGuidedUnproven : GuidedProofDecode(rec.pad[0]));
    }
  }
};

template <int G>
Session* MakeProve(int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes, int width,
                   float c_puct, int tactics, long long tactics_nodes, int flags, uint8_t* obs, uint8_t* mask,
                   uint8_t* status, int* rc) {
  if (simulations < 1 || simulations > kSearchMaxSimulations || nodes < simulations + 1 || nodes > kGuidedMaxNodes ||
      width < 1 || width > kGuidedMaxWidth || tactics < 0 || tactics > kGuidedMaxTactics || tactics_nodes < 1 ||
      tactics_nodes > kGuidedMaxTacticsNodes || (flags & ~kGuidedProve) != 0) {
    *rc = -6;
    return nullptr;
  }
  ProveRun<G>* r = new ProveRun<G>(n, simulations, nodes, width, c_puct, tactics, tactics_nodes, flags);
  *rc = r->Begin(hidden, done, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

// A session as pgx_tactics_begin's with a flags word (kGuidedProve; 0: that session).  It is advanced, read, rerooted
// and ended through pgx_wide_advance / _result / _reroot / _end and pgx_tactics_decided.  *rc as pgx_tactics_begin; -6
// also for a flags bit that is not known.
void* pgx_prove_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes,
                      int width, float c_puct, int tactics, long long tactics_nodes, int flags, uint8_t* obs,
                      uint8_t* mask, uint8_t* status, int* rc) {
#define EPA_MAKE(G) \
  MakeProve<G>(n, hidden, done, simulations, nodes, width, c_puct, tactics, tactics_nodes, flags, obs, mask, status, rc)
  switch (game) {
    case kTicTacToe: return EPA_MAKE(kTicTacToe);
    case kConnectFour: return EPA_MAKE(kConnectFour);
    case kHex: return EPA_MAKE(kHex);
    case kOthello: return EPA_MAKE(kOthello);
    default: *rc = -1; return nullptr;
  }
#undef EPA_MAKE
}

// value [n] and q [n * A]
void pgx_prove_proof(void* session, int8_t* value, int8_t* q) {
  dynamic_cast<ProveSession*>(static_cast<Session*>(session))->Proof(value, q);
}

int pgx_prove_limits(int which) { return which == 0 ? kGuidedProve : kGuidedUnproven; }

}  // extern "C"

#ifdef PGX_PROVE_MAIN
#include <cstdio>

// Three rounds of one session per game (ConnectFour 4 roots some plies in, D = 2; Othello 4 roots late in the game,
// D = 0; W = 4, S = 24) with a constant evaluator and a reroot by the chosen move between the rounds: an ordinary
// process for the host sanitizers.
template <int G>
int Play(int plies, int tactics) {
  constexpr int A = Dims<G>::A, OB = Dims<G>::H * Dims<G>::W * Dims<G>::C, HW = HiddenWords<G>();
  const int n = 4, S = 24, W = 4, C = 3 * S + 1;
  std::vector<int32_t> hidden((size_t)n * HW);
  std::vector<uint8_t> done((size_t)n, 0), o1(OB), m1(A);
  for (int i = 0; i < n; ++i) {
    State s{};
    s.done = 1;
    struct Gen {
      uint32_t x;
      uint32_t Next() { return x = x * 1664525u + 1013904223u; }
    } rng{(uint32_t)(7 + i)};
    Reset<G>(rng, s);
    std::vector<int32_t> w(HW), w2(HW);
    Hidden<G>(s, w.data());
    int32_t info[4];
    uint32_t x = 99u + (uint32_t)i;
    for (int ply = 0; ply < plies + i; ++ply) {  // a legal move by a small generator; stop one ply before the end
      if (pgx_tactics_step(G, w.data(), -1, w2.data(), o1.data(), m1.data(), info) != 0) return 10;
      int legal = 0;
      for (int a = 0; a < A; ++a) legal += m1[a];
      if (legal == 0) break;
      x = x * 1664525u + 1013904223u;
      int pick = (int)((x >> 8) % (uint32_t)legal), a = 0;
      for (; a < A; ++a) {
        if (m1[a] && pick-- == 0) break;
      }
      if (pgx_tactics_step(G, w.data(), a, w2.data(), o1.data(), m1.data(), info) != 0 || info[0]) break;
      w = w2;
    }
    std::memcpy(hidden.data() + (size_t)i * HW, w.data(), sizeof(int32_t) * HW);
  }
  std::vector<uint8_t> obs((size_t)n * W * OB), mask((size_t)n * W * A), status((size_t)n * W);
  int rc = -9;
  void* h = pgx_prove_begin(G, n, hidden.data(), done.data(), S, C, W, 1.25f, tactics, 4096, kGuidedProve, obs.data(),
                            mask.data(), status.data(), &rc);
  if (h == nullptr || rc != 0) return 1;
  std::vector<float> priors((size_t)n * W * A), values((size_t)n * W, 0.0f);
  std::vector<int32_t> visits((size_t)n * A), action(n), used(n), sims(n);
  std::vector<float> vals((size_t)n * A);
  std::vector<int8_t> value(n), q((size_t)n * A);
  for (int round = 0; round < 3; ++round) {
    for (int t = 0; t <= S; ++t) {
      for (size_t r = 0; r < (size_t)n * W; ++r) {
        int legal = 0;
        for (int a = 0; a < A; ++a) legal += mask[r * A + a];
        for (int a = 0; a < A; ++a) priors[r * A + a] = mask[r * A + a] ? 1.0f / (float)legal : 0.0f;
      }
      if (pgx_wide_advance(h, priors.data(), values.data(), obs.data(), mask.data(), status.data()) != 0) return 2;
    }
    pgx_wide_result(h, visits.data(), vals.data(), action.data(), used.data(), sims.data());
    pgx_prove_proof(h, value.data(), q.data());
    for (int i = 0; i < n; ++i) {
      std::printf("game %d round %d root %d: action %d, %d nodes, %d simulations, proof %d\n", G, round, i, action[i],
                  used[i], sims[i], (int)value[i]);
      if (action[i] < 0) action[i] = 0;
    }
    if (round < 2 && pgx_wide_reroot(h, action.data(), S, obs.data(), mask.data(), status.data()) != 0) return 3;
  }
  pgx_wide_end(h);
  return 0;
}

int main() {
  const int a = Play<kConnectFour>(14, 2);
  if (a != 0) return a;
  return Play<kOthello>(52, 0);
}
#endif
