// MiniGrid navigation tasks: per-env reset / step / observation, written once as __host__ __device__ code.
//
// The step kernel (minigrid.hip) runs it one env per lane over a grid kept in HBM; the host harness
// (tests/cpu_harness/minigrid_host.cpp) compiles the same source with g++ and replays the fixtures.
// Restates, for the seven classic navigation env_names of the reference:
//   MiniGridTask::{Reset,Step,PlaceObj,PlaceAgent,RandInt,SuccessReward}  minigrid/impl/minigrid_core.cc:51-291
//   MiniGridTask::GenImage (view window, rotations, visibility sweep)       minigrid/impl/minigrid_render.cc:276-369
//   EmptyTask, DoorKeyTask, DistShiftTask, LavaGapTask, CrossingTask,
//   DynamicObstaclesTask                                                    minigrid/impl/minigrid_tasks.cc:27-255
//   FourRoomsTask                                                           minigrid/impl/minigrid_room_tasks.cc:222-252
//   WorldObj encoding, CanSeeBehind, CanOverlap, CanPickup, door states     minigrid/impl/utils.h:200-270
//
// A cell is one 16-bit word: bits 0-3 type, 4-6 colour, 7-8 state (door: 0 open, 1 closed, 2 locked), i.e.
// exactly what WorldObj::Encode() reports.  None of these tasks puts an object inside a box, so the word is
// the whole cell.  The carried object is one more word (an empty cell when nothing is carried).
//
// The generator G supplies the reference's draws from the env's std::mt19937:
//   int  G::UniformInt(int a, int b)                        uniform_int_distribution<int>(a, b)
//   void G::UniformPair(uint32 b0, uint32 b1, int*, int*)   std::__gen_two_uniform_ints(b0, b1, g)
// (device: MgGen over Mt19937, minigrid.hip).  Every rejection loop is bounded by TaskCfg::max_tries; when a
// bound is exhausted Reset returns false (the reference throws, or -- with its unbounded default -- spins).
#ifndef ENVPOOL_AMD_CSRC_MINIGRID_ENV_HIP_H_
#define ENVPOOL_AMD_CSRC_MINIGRID_ENV_HIP_H_

#include <cstdint>

#if defined(__HIPCC__)
#define MG_HD __host__ __device__
#else
#define MG_HD
#endif
// loops kept rolled on the device: unrolled copies of the reset's draw loops only add register pressure
#if defined(__HIP_DEVICE_COMPILE__)
#define MG_ROLLED _Pragma("unroll 1")
#else
#define MG_ROLLED
#endif

namespace epa {
namespace mg {

enum : int { kUnseen = 0, kEmpty, kWall, kFloor, kDoor, kKey, kBall, kBox, kGoal, kLava, kAgent };
enum : int { kRed = 0, kGreen, kBlue, kPurple, kYellow, kGrey };
enum : int { kLeft = 0, kRight, kForward, kPickup, kDrop, kToggle, kDone };
// env_name codes (engine key "env_name_code", envpool_amd/minigrid/__init__.py)
enum Task : int { kTaskEmpty = 0, kTaskDoorKey, kTaskDistShift, kTaskCrossing, kTaskLavaGap, kTaskDynObs,
                  kTaskFourRooms };

constexpr int kView = 7;          // agent_view_size of every task here
constexpr int kImageBytes = kView * kView * 3;
constexpr int kMissionBytes = 96;
constexpr int kMaxSide = 19;      // FourRooms
constexpr int kMaxCells = kMaxSide * kMaxSide;
constexpr int kMaxObstacles = 8;  // Dynamic-Obstacles-16x16 (grid sides <= 16)

MG_HD constexpr uint16_t MakeCell(int type, int color, int state = 0) {
  return (uint16_t)(type | (color << 4) | (state << 7));
}
constexpr uint16_t kEmptyCell = MakeCell(kEmpty, kRed);  // WorldObj(kEmpty): DefaultColor(kEmpty) = kRed
constexpr uint16_t kWallCell = MakeCell(kWall, kGrey);
constexpr uint16_t kGoalCell = MakeCell(kGoal, kGreen);
constexpr uint16_t kLavaCell = MakeCell(kLava, kRed);
constexpr uint16_t kBallCell = MakeCell(kBall, kBlue);
constexpr uint16_t kKeyCell = MakeCell(kKey, kYellow);
constexpr uint16_t kLockedDoorCell = MakeCell(kDoor, kYellow, 2);

MG_HD inline int TypeOf(uint16_t c) { return c & 15; }
MG_HD inline int ColorOf(uint16_t c) { return (c >> 4) & 7; }
MG_HD inline int StateOf(uint16_t c) { return (c >> 7) & 3; }
MG_HD inline bool CanSeeBehind(uint16_t c) {  // utils.h:200-210
  const int t = TypeOf(c);
  return t == kDoor ? StateOf(c) == 0 : t != kWall;
}
MG_HD inline bool CanOverlap(uint16_t c) {  // utils.h:212-225
  const int t = TypeOf(c);
  if (t == kDoor) return StateOf(c) == 0;
  return !(t == kWall || t == kKey || t == kBall || t == kBox);
}
MG_HD inline bool CanPickup(uint16_t c) {
  const int t = TypeOf(c);
  return t == kKey || t == kBall || t == kBox;
}

// Task properties fixed by the task alone, used both where the host derives a TaskCfg (MakeTaskCfg) and in
// the kernel's per-task instantiation (where they fold to constants):
//   see_through_walls_ of the task's constructor (minigrid_tasks.cc:28, :67, :196: Empty, DistShift,
//   DynamicObstacles), FourRooms' fixed 19 x 19 grid (minigrid_room_tasks.cc:223), obstacles only in
//   DynamicObstacles
MG_HD constexpr bool SeeThroughWalls(int task) {
  return task == kTaskEmpty || task == kTaskDistShift || task == kTaskDynObs;
}
MG_HD constexpr bool HasFixedSide(int task) { return task == kTaskFourRooms; }
MG_HD constexpr bool HasObstacles(int task) { return task == kTaskDynObs; }

// Numeric task parameters (the reference's config keys that select and shape the task).
struct TaskCfg {
  int task;
  int width, height;       // grid size (size x size except DistShift)
  int size;
  int start_x, start_y, start_dir;  // agent_start_pos / agent_start_dir (x < 0: random start)
  int num_crossings;
  int obstacle;            // obstacle_type as a cell word (lava or wall)
  int strip2_row;
  int n_obstacles;         // DynamicObstaclesTask's clamped count
  int max_steps;           // max_episode_steps
  int max_tries;           // engine bound on every rejection loop ("minigrid_max_tries")
  int see_through;         // see_through_walls_
};

// One env's state outside the grid.
struct EnvState {
  int ax, ay, dir;
  uint16_t carry;
  uint64_t obst;  // DynamicObstacles: byte i = obstacle i's x | y << 4 (sides <= 16)
};
MG_HD inline int ObstX(uint64_t o, int i) { return (int)((o >> (8 * i)) & 15u); }
MG_HD inline int ObstY(uint64_t o, int i) { return (int)((o >> (8 * i + 4)) & 15u); }
MG_HD inline uint64_t SetObst(uint64_t o, int i, int x, int y) {
  return (o & ~(255ull << (8 * i))) | ((uint64_t)(x | (y << 4)) << (8 * i));
}

// Grid of one env: cell (x, y) at p[y * width + x].
struct GridRef {
  uint16_t* p;
  int w;
  MG_HD uint16_t Get(int x, int y) const { return p[y * w + x]; }
  MG_HD void Set(int x, int y, uint16_t c) const { p[y * w + x] = c; }
};

MG_HD inline void HorzWall(const GridRef& g, int x, int y, int len, uint16_t c) {
  for (int i = 0; i < len; ++i) g.Set(x + i, y, c);
}
MG_HD inline void VertWall(const GridRef& g, int x, int y, int len, uint16_t c) {
  for (int j = 0; j < len; ++j) g.Set(x, y + j, c);
}
MG_HD inline void ClearWalled(const GridRef& g, int w, int h) {  // ClearGrid + WallRect(0, 0, w, h)
  for (int i = 0; i < w * h; ++i) g.p[i] = kEmptyCell;
  HorzWall(g, 0, 0, w, kWallCell);
  HorzWall(g, 0, h - 1, w, kWallCell);
  VertWall(g, 0, 0, h, kWallCell);
  VertWall(g, w - 1, 0, h, kWallCell);
}

// MiniGridTask::PlaceObj (minigrid_core.cc:225-260) without a reject function: returns false when more than
// `max_tries` draws were rejected.  RandInt(lo, hi) is uniform_int_distribution<>(lo, hi - 1); x before y.
template <typename G>
MG_HD inline bool PlaceObj(G& rng, const GridRef& g, const TaskCfg& c, const EnvState& s, int top_x, int top_y,
                           int size_x, int size_y, int max_tries, uint16_t obj, int* px, int* py) {
  top_x = top_x > 0 ? top_x : 0;
  top_y = top_y > 0 ? top_y : 0;
  const int hx = (top_x + size_x < c.width ? top_x + size_x : c.width) - 1;
  const int hy = (top_y + size_y < c.height ? top_y + size_y : c.height) - 1;
  for (int tries = 0;; ++tries) {
    if (tries > max_tries) return false;
    const int x = rng.UniformInt(top_x, hx);
    const int y = rng.UniformInt(top_y, hy);
    if (TypeOf(g.Get(x, y)) != kEmpty) continue;
    if (x == s.ax && y == s.ay) continue;
    g.Set(x, y, obj);
    *px = x;
    *py = y;
    return true;
  }
}

// MiniGridTask::PlaceAgent (:262-276): agent_pos_ = (-1, -1) during the search, then a direction draw.
template <typename G>
MG_HD inline bool PlaceAgent(G& rng, const GridRef& g, const TaskCfg& c, EnvState& s, int top_x, int top_y,
                             int size_x, int size_y) {
  s.ax = s.ay = -1;
  int x, y;
  if (!PlaceObj(rng, g, c, s, top_x, top_y, size_x, size_y, c.max_tries, kEmptyCell, &x, &y)) return false;
  s.ax = x;
  s.ay = y;
  s.dir = rng.UniformInt(0, 3);
  return true;
}

// std::shuffle of libstdc++ 11 (bits/stl_algo.h:3743-3780) over n <= 16 nibbles of `v`, for a generator whose
// range (2^32 - 1) is at least n^2: an even n swaps element 1 with a uniform_int<>(0, 1) draw first, then the
// rest go in pairs, both swap positions from ONE draw (__gen_two_uniform_ints, :3706).
MG_HD inline int Nib(uint64_t v, int j) { return (int)((v >> (4 * j)) & 15u); }
MG_HD inline uint64_t SetNib(uint64_t v, int j, int x) {
  return (v & ~(15ull << (4 * j))) | ((uint64_t)x << (4 * j));
}
MG_HD inline uint64_t SwapNib(uint64_t v, int i, int j) {
  const int a = Nib(v, i), b = Nib(v, j);
  return SetNib(SetNib(v, i, b), j, a);
}
template <typename G>
MG_HD inline uint64_t ShuffleNibbles(G& rng, uint64_t v, int n) {
  if (n == 0) return v;
  int i = 1;
  if ((n % 2) == 0) {
    v = SwapNib(v, i, rng.UniformInt(0, 1));
    ++i;
  }
  MG_ROLLED
  while (i != n) {
    const uint32_t r = (uint32_t)i + 1u;
    int p0, p1;
    rng.UniformPair(r, r + 1u, &p0, &p1);
    v = SwapNib(v, i, p0);
    ++i;
    v = SwapNib(v, i, p1);
    ++i;
  }
  return v;
}
// value of the m-th limit of CrossingTask: 0, the set bits of `mask` (river coordinate 2 b) ascending, side - 1
MG_HD inline int Limit(uint32_t mask, int count, int m, int side) {
  if (m == 0) return 0;
  if (m > count) return side - 1;
  MG_ROLLED
  for (int b = 0; b < 16; ++b) {
    if ((mask >> b) & 1u) {
      if (--m == 0) return 2 * b;
    }
  }
  return side - 1;
}

// The task's GenGrid (MiniGridTask::Reset: step count 0, nothing carried).  false: a rejection bound ran out.
template <typename G>
MG_HD inline bool ResetEnv(G& rng, const GridRef& g, const TaskCfg& c, EnvState& s) {
  s.carry = kEmptyCell;
  s.obst = 0;
  s.ax = s.ay = -1;
  s.dir = 0;
  const int W = c.width, H = c.height, n = c.size;
  switch (c.task) {
    case kTaskEmpty:  // minigrid_tasks.cc:34-46
    case kTaskDynObs:  // :203-219
      ClearWalled(g, n, n);
      g.Set(n - 2, n - 2, kGoalCell);
      if (c.start_x >= 0) {
        s.ax = c.start_x;
        s.ay = c.start_y;
        s.dir = c.start_dir;
      } else if (c.task == kTaskEmpty) {
        if (!PlaceAgent(rng, g, c, s, 1, 1, n - 2, n - 2)) return false;
      } else {
        if (!PlaceAgent(rng, g, c, s, 0, 0, W, H)) return false;
      }
      if (c.task == kTaskDynObs) {
        const int tries = c.max_tries < 100 ? c.max_tries : 100;
        s.obst = 0;
        MG_ROLLED
        for (int i = 0; i < c.n_obstacles; ++i) {
          int x, y;
          if (!PlaceObj(rng, g, c, s, 0, 0, W, H, tries, kBallCell, &x, &y)) return false;
          s.obst = SetObst(s.obst, i, x, y);
        }
      }
      return true;
    case kTaskDoorKey: {  // :51-63
      ClearWalled(g, n, n);
      g.Set(n - 2, n - 2, kGoalCell);
      const int split = rng.UniformInt(2, n - 3);
      VertWall(g, split, 0, n, kWallCell);
      if (!PlaceAgent(rng, g, c, s, 0, 0, split, n)) return false;
      const int door = rng.UniformInt(1, n - 3);
      g.Set(split, door, kLockedDoorCell);
      int x, y;
      return PlaceObj(rng, g, c, s, 0, 0, split, n, c.max_tries, kKeyCell, &x, &y);
    }
    case kTaskDistShift:  // :75-90
      ClearWalled(g, W, H);
      g.Set(W - 2, 1, kGoalCell);
      for (int i = 0; i < W - 6; ++i) {
        g.Set(3 + i, 1, kLavaCell);
        g.Set(3 + i, c.strip2_row, kLavaCell);
      }
      if (c.start_x >= 0) {
        s.ax = c.start_x;
        s.ay = c.start_y;
        s.dir = c.start_dir;
        return true;
      }
      return PlaceAgent(rng, g, c, s, 0, 0, W, H);
    case kTaskLavaGap: {  // :98-115
      ClearWalled(g, n, n);
      s.ax = s.ay = 1;
      g.Set(n - 2, n - 2, kGoalCell);
      const int gx = rng.UniformInt(2, n - 3);
      const int gy = rng.UniformInt(1, n - 2);
      VertWall(g, gx, 1, n - 2, (uint16_t)c.obstacle);
      g.Set(gx, gy, kEmptyCell);
      return true;
    }
    case kTaskCrossing: {  // :122-195
      ClearWalled(g, n, n);
      s.ax = s.ay = 1;
      g.Set(n - 2, n - 2, kGoalCell);
      // rivers (vertical?, i) for i = 2, 4, .. < n - 2, as nibbles (i / 2 - 1) | vertical << 3
      uint64_t rivers = 0;
      int nr = 0;
      for (int i = 2; i < n - 2; i += 2) {
        rivers = SetNib(rivers, nr++, (i / 2 - 1) | 8);
        rivers = SetNib(rivers, nr++, i / 2 - 1);
      }
      rivers = ShuffleNibbles(rng, rivers, nr);
      uint32_t vmask = 0, hmask = 0;  // bit b: a river at 2 b (the sorted lists rivers_v / rivers_h)
      int nv = 0, nh = 0;
      for (int j = 0; j < c.num_crossings; ++j) {
        const int r = Nib(rivers, j);
        const int b = (r & 7) + 1;
        if (r & 8) {
          vmask |= 1u << b;
          ++nv;
        } else {
          hmask |= 1u << b;
          ++nh;
        }
      }
      MG_ROLLED
      for (int b = 0; b < 16; ++b) {
        if ((hmask >> b) & 1u) HorzWall(g, 1, 2 * b, n - 2, (uint16_t)c.obstacle);
      }
      MG_ROLLED
      for (int b = 0; b < 16; ++b) {
        if ((vmask >> b) & 1u) VertWall(g, 2 * b, 1, n - 2, (uint16_t)c.obstacle);
      }
      uint64_t path = 0;  // nv trues, then nh falses
      for (int j = 0; j < nv + nh; ++j) path = SetNib(path, j, j < nv ? 1 : 0);
      path = ShuffleNibbles(rng, path, nv + nh);
      int ri = 0, rj = 0;
      MG_ROLLED
      for (int j = 0; j < nv + nh; ++j) {
        int x, y;
        if (Nib(path, j)) {
          x = Limit(vmask, nv, ri + 1, n);
          y = rng.UniformInt(Limit(hmask, nh, rj, n) + 1, Limit(hmask, nh, rj + 1, n) - 1);
          ++ri;
        } else {
          x = rng.UniformInt(Limit(vmask, nv, ri, n) + 1, Limit(vmask, nv, ri + 1, n) - 1);
          y = Limit(hmask, nh, rj + 1, n);
          ++rj;
        }
        g.Set(x, y, kEmptyCell);
      }
      return true;
    }
    default: {  // kTaskFourRooms, minigrid_room_tasks.cc:225-252
      for (int i = 0; i < W * H; ++i) g.p[i] = kEmptyCell;
      HorzWall(g, 0, 0, W, kWallCell);
      HorzWall(g, 0, H - 1, W, kWallCell);
      VertWall(g, 0, 0, H, kWallCell);
      VertWall(g, W - 1, 0, H, kWallCell);
      const int rw = W / 2, rh = H / 2;
      for (int j = 0; j < 2; ++j) {
        for (int i = 0; i < 2; ++i) {
          const int xl = i * rw, yt = j * rh, xr = xl + rw, yb = yt + rh;
          if (i + 1 < 2) {
            VertWall(g, xr, yt, rh, kWallCell);
            g.Set(xr, rng.UniformInt(yt + 1, yb - 1), kEmptyCell);
          }
          if (j + 1 < 2) {
            HorzWall(g, xl, yb, rw, kWallCell);
            g.Set(rng.UniformInt(xl + 1, xr - 1), yb, kEmptyCell);
          }
        }
      }
      if (!PlaceAgent(rng, g, c, s, 0, 0, W, H)) return false;
      int x, y;
      return PlaceObj(rng, g, c, s, 0, 0, W, H, c.max_tries, kGoalCell, &x, &y);
    }
  }
}

// MiniGridTask::SuccessReward (:291): float32 1 - 0.9 * (step_count / max_steps), no contraction.
MG_HD inline float SuccessReward(int step_count, int max_steps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float q = (float)step_count / (float)max_steps;
  const float m = 0.9f * q;
  return 1.0f - m;
}

// MiniGridTask::Step (:71-147) with DynamicObstaclesTask::{BeforeStep, AfterStep} (:221-247); `step_count`
// is the count after this step.  Returns the reward, sets *terminated (max_steps included).
template <typename G>
MG_HD inline float StepEnv(G& rng, const GridRef& g, const TaskCfg& c, EnvState& s, int act, int step_count,
                           bool* terminated) {
  float reward = 0.0f;
  bool term = false;
  // DIR_TO_VEC: (1, 0), (0, 1), (-1, 0), (0, -1)
  const int fx = s.ax + (s.dir == 0 ? 1 : s.dir == 2 ? -1 : 0), fy = s.ay + (s.dir == 1 ? 1 : s.dir == 3 ? -1 : 0);
  const uint16_t pre_fwd = g.Get(fx, fy);
  bool pre_front_blocked = false;
  if (c.task == kTaskDynObs) {
    pre_front_blocked = act == kForward && TypeOf(pre_fwd) != kGoal && TypeOf(pre_fwd) != kEmpty;
    MG_ROLLED
    for (int i = 0; i < c.n_obstacles; ++i) {
      const int ox = ObstX(s.obst, i), oy = ObstY(s.obst, i);
      const int tx = ox - 1 > 0 ? ox - 1 : 0, ty = oy - 1 > 0 ? oy - 1 : 0;
      const int ex = ox + 2 < c.width ? ox + 2 : c.width, ey = oy + 2 < c.height ? oy + 2 : c.height;
      for (int attempt = 0; attempt < 100; ++attempt) {
        const int x = rng.UniformInt(tx, ex - 1);
        const int y = rng.UniformInt(ty, ey - 1);
        if (TypeOf(g.Get(x, y)) != kEmpty || (x == s.ax && y == s.ay)) continue;
        g.Set(x, y, kBallCell);
        g.Set(ox, oy, kEmptyCell);
        s.obst = SetObst(s.obst, i, x, y);
        break;
      }
    }
  }
  if (act == kLeft) {
    s.dir = (s.dir + 3) % 4;
  } else if (act == kRight) {
    s.dir = (s.dir + 1) % 4;
  } else if (act == kForward) {
    const uint16_t cur = g.Get(fx, fy);
    if (CanOverlap(cur)) {
      s.ax = fx;
      s.ay = fy;
    }
    if (TypeOf(cur) == kGoal) {
      reward = SuccessReward(step_count, c.max_steps);
      term = true;
    } else if (TypeOf(cur) == kLava) {
      term = true;
    }
  } else if (act == kPickup) {
    const uint16_t cur = g.Get(fx, fy);
    if (TypeOf(s.carry) == kEmpty && CanPickup(cur)) {
      s.carry = cur;
      g.Set(fx, fy, kEmptyCell);
    }
  } else if (act == kDrop) {
    if (TypeOf(s.carry) != kEmpty && TypeOf(g.Get(fx, fy)) == kEmpty) {
      g.Set(fx, fy, s.carry);
      s.carry = kEmptyCell;
    }
  } else if (act == kToggle) {
    const uint16_t cur = g.Get(fx, fy);
    if (TypeOf(cur) == kDoor) {
      const int st = StateOf(cur);
      if (st == 2) {  // locked: opens with a key of its colour
        if (TypeOf(s.carry) == kKey && ColorOf(s.carry) == ColorOf(cur)) {
          g.Set(fx, fy, MakeCell(kDoor, ColorOf(cur), 0));
        }
      } else {
        g.Set(fx, fy, MakeCell(kDoor, ColorOf(cur), st == 0 ? 1 : 0));
      }
    } else if (TypeOf(cur) == kBox) {  // (no box holds anything in these tasks)
      g.Set(fx, fy, kEmptyCell);
    }
  }
  if (c.task == kTaskDynObs && act == kForward && pre_front_blocked) {
    reward = -1.0f;
    term = true;
  }
  if (step_count >= c.max_steps) term = true;
  *terminated = term;
  return reward;
}

// MiniGridTask::GenImage (minigrid_render.cc:276-369) into img[(x * 7 + y) * 3 + ch] (obs(x, y, ch), x-major).
MG_HD inline void GenImage(const GridRef& g, const TaskCfg& c, const EnvState& s, uint8_t* img) {
  const int half = kView / 2;
  int top_x, top_y;
  if (s.dir == 0) {
    top_x = s.ax;
    top_y = s.ay - half;
  } else if (s.dir == 1) {
    top_x = s.ax - half;
    top_y = s.ay;
  } else if (s.dir == 2) {
    top_x = s.ax - kView + 1;
    top_y = s.ay - half;
  } else {
    top_x = s.ax - half;
    top_y = s.ay - kView + 1;
  }
  // view cell (y, x) after dir + 1 rotations (rotated[v - 1 - x][y] = view[y][x]) comes from window cell
  // (y', x') found by applying (y, x) -> (x, v - 1 - y) dir + 1 times
  auto src = [&](int y, int x) -> uint16_t {
    for (int r = 0; r <= s.dir; ++r) {
      const int t = y;
      y = x;
      x = kView - 1 - t;
    }
    const int gx = top_x + x, gy = top_y + y;
    return (gx >= 0 && gx < c.width && gy >= 0 && gy < c.height) ? g.Get(gx, gy) : kWallCell;
  };
  // visibility: bit y * 7 + x (the window is read twice instead of being held: no 49-word array per lane)
  uint64_t vis;
  const int agx = half, agy = kView - 1;
  if (c.see_through) {
    vis = (1ull << (kView * kView)) - 1;
  } else {
    uint64_t see = 0;
    for (int y = 0; y < kView; ++y) {
      for (int x = 0; x < kView; ++x) {
        if (CanSeeBehind(src(y, x))) see |= 1ull << (y * kView + x);
      }
    }
    vis = 1ull << (agy * kView + agx);
    auto on = [&](int x, int y) { return ((vis >> (y * kView + x)) & (see >> (y * kView + x)) & 1ull) != 0; };
    auto set = [&](int x, int y) { vis |= 1ull << (y * kView + x); };
    for (int y = kView - 1; y >= 0; --y) {
      for (int x = 0; x < kView - 1; ++x) {
        if (!on(x, y)) continue;
        set(x + 1, y);
        if (y > 0) {
          set(x + 1, y - 1);
          set(x, y - 1);
        }
      }
      for (int x = kView - 1; x >= 1; --x) {
        if (!on(x, y)) continue;
        set(x - 1, y);
        if (y > 0) {
          set(x - 1, y - 1);
          set(x, y - 1);
        }
      }
    }
  }
  // the agent's own cell shows what it carries (an empty cell when nothing)
  for (int x = 0; x < kView; ++x) {
    for (int y = 0; y < kView; ++y) {
      uint8_t* o = img + (x * kView + y) * 3;
      const bool seen = (vis >> (y * kView + x)) & 1ull;
      const uint16_t v = !seen ? 0 : (x == agx && y == agy) ? s.carry : src(y, x);
      o[0] = (uint8_t)TypeOf(v);
      o[1] = (uint8_t)ColorOf(v);
      o[2] = (uint8_t)StateOf(v);
    }
  }
}

}  // namespace mg
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_MINIGRID_ENV_HIP_H_
