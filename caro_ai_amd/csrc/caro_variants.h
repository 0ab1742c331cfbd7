// caro_variants.h -- the lane geometries of the tree kernels and the run-time choice among them: one table for the
// kernels (caro_engine.hip), the host-side single-state helpers (caro_host.inc) and the CPU sanitizer build of those
// helpers (oracle/asan/host_tu.cpp, plain g++).  Needs caro_rules.h and include/caro_hip.h.
#ifndef CARO_VARIANTS_H
#define CARO_VARIANTS_H

#include "../../include/caro_noise.h"

namespace caro {

template <class R_, int LPD_, int APL_>
struct Geo {
  using R = R_;
  static constexpr int LPD = LPD_, APL = APL_, AP = LPD_ * APL_, KW = R_::KW;
};
using GeoC4 = Geo<C4Rules, 8, 1>;
using GeoM16 = Geo<MnkRules<1>, 16, 1>;
using GeoM32 = Geo<MnkRules<1>, 32, 1>;
using GeoM64 = Geo<MnkRules<1>, 64, 1>;
using GeoM128 = Geo<MnkRules<2>, 64, 2>;
using GeoM256 = Geo<MnkRules<4>, 64, 4>;
// caro: the m,n,k geometry of the same A, with the caro win test (a type of its own: the m,n,k kernels stay as they are)
using GeoK16 = Geo<CaroRules<1>, 16, 1>;
using GeoK32 = Geo<CaroRules<1>, 32, 1>;
using GeoK64 = Geo<CaroRules<1>, 64, 1>;
using GeoK128 = Geo<CaroRules<2>, 64, 2>;
using GeoK256 = Geo<CaroRules<4>, 64, 4>;

enum Variant { V_C4, V_M16, V_M32, V_M64, V_M128, V_M256, V_K16, V_K32, V_K64, V_K128, V_K256, V_BAD };

static inline Variant pick_variant(int kind, int n) {
  if (kind == CARO_GAME_CONNECT4) return V_C4;
  if ((kind != CARO_GAME_MNK && kind != CARO_GAME_CARO) || n < 2 || n > 15) return V_BAD;
  const int A = n * n;
  const bool caro = kind == CARO_GAME_CARO;
  if (A <= 16) return caro ? V_K16 : V_M16;
  if (A <= 32) return caro ? V_K32 : V_M32;
  if (A <= 64) return caro ? V_K64 : V_M64;
  if (A <= 128) return caro ? V_K128 : V_M128;
  return caro ? V_K256 : V_M256;
}
static inline int variant_kw(Variant v) {
  switch (v) {
    case V_C4: return 1;
    case V_M16: case V_M32: case V_M64: case V_K16: case V_K32: case V_K64: return 2;
    case V_M128: case V_K128: return 4;
    case V_M256: case V_K256: return 8;
    default: return 0;
  }
}
static inline int variant_lpd(Variant v) {
  switch (v) {
    case V_C4: return 8;
    case V_M16: case V_K16: return 16;
    case V_M32: case V_K32: return 32;
    default: return 64;
  }
}
static inline int variant_ap(Variant v) {
  switch (v) {
    case V_C4: return 8;
    case V_M16: case V_K16: return 16;
    case V_M32: case V_K32: return 32;
    case V_M64: case V_K64: return 64;
    case V_M128: case V_K128: return 128;
    case V_M256: case V_K256: return 256;
    default: return 0;
  }
}
static inline GameParams make_gp(int kind, int n, int k) {
  GameParams gp;
  gp.kind = kind;
  if (kind == CARO_GAME_CONNECT4) {
    gp.n = 0; gp.k = 4; gp.A = 7; gp.rows = 6; gp.cols = 7;
  } else {
    gp.n = n; gp.k = k; gp.A = n * n; gp.rows = n; gp.cols = n;
  }
  return gp;
}

// The opening rule of include/caro_hip.h ("openings"), one statement for the engine's four game starts, the batched
// kernel (caro_openings_batch) and the host helper (caro_host_opening): a single thread, from the initial position with
// `player` to move.  On return `b` / `player` are the game's root and its mover; the value is the plies made.
// (At most max_plies <= 64 rounds of two passes over the A actions, once per game.)
template <class R>
CR_HD int opening_position(const GameParams& gp, uint64_t seed, uint64_t uid, int max_plies, typename R::Board& b,
                           int& player) {
  b = R::initial(gp);
  int r = (int)(caro_open_uniform(seed, uid, 0u) * (double)(max_plies + 1));
  r = r < max_plies ? r : max_plies;
  int made = 0;
  for (int i = 0; i < r; ++i) {
    int L = 0;
    for (int a = 0; a < gp.A; ++a) L += R::legal(gp, b, a) ? 1 : 0;
    int j = (int)(caro_open_uniform(seed, uid, (uint32_t)(1 + i)) * (double)L);
    j = j < L - 1 ? j : L - 1;
    int mv = 0;
    for (int a = 0, c = 0; a < gp.A; ++a)
      if (R::legal(gp, b, a)) {
        mv = c == j ? a : mv;
        ++c;
      }
    typename R::Board nb = b;
    if (R::move(gp, nb, mv, player) || R::full(gp, nb)) break;  // a move that would end the game is not made
    b = nb;
    player = 1 - player;
    ++made;
  }
  return made;
}

// The two rules of include/caro_hip.h ("forced playouts"), one statement for the tree kernels (the root level of a
// descent, the ply) and the host helpers (caro_host_forced_root / caro_host_forced_prune).  Float64, in the order the
// header gives; no contraction (the engine is compiled with -ffp-contract=off, and nothing here can be fused on a host).
// fp_forced: is an action with n visits and noised prior `prob` forced at a root whose row sums to T?
CR_HD bool fp_forced(int n, int T, double prob, double k) {
  return n > 0 && (double)n * (double)n < (k * prob) * (double)T;
}
// the root score of an edge with n visits as the pruning rule forms it (no noise: P is the raw prior)
CR_HD double fp_score(double q, double c, double p, double sq, int n) {
  return q + ((c * p) * sq) / (double)(1 + n);
}
// N' of one action a != b with n > 0 visits: the smallest count in [max(0, n - F), n] whose score is below sstar (the
// predicate is monotone in the count: the first true one by bisection), n itself if there is none; a lone visit is dropped.
CR_HD int fp_pruned(int n, double q, double p, double c, double k, int T, double sq, double sstar) {
  int hi = n;
  if (fp_score(q, c, p, sq, n) < sstar) {
    const int F = (int)caro_sqrt((k * p) * (double)T);
    int lo = n - F > 0 ? n - F : 0;
    while (lo < hi) {  // invariant: the predicate holds at hi and at nothing below lo
      const int mid = lo + (hi - lo) / 2;
      if (fp_score(q, c, p, sq, mid) < sstar) hi = mid;
      else lo = mid + 1;
    }
  }
  return hi == 1 ? 0 : hi;
}

// The per-action pieces of include/caro_hip.h ("first-play urgency"), one statement for descend_level and
// caro_host_fpu_level.  fpu_mass: m_a, the prior of a visited action as an integer multiple of 2^-22 (the clamp sends a
// NaN to 0; the product with 2^22 is exact).  fpu_visited_sqrt: s from the integer sum M of the m_a.  fpu_q_root /
// fpu_q: the Q an unvisited action gets at the root level (float64) and below it (one rounding to float32): the
// product, then the difference, in float64.  No contraction, as above.
CR_HD int fpu_mass(float p) {
  float c = p > 0.0f ? p : 0.0f;
  c = c < 1.0f ? c : 1.0f;
  return (int)__builtin_floorf(c * 4194304.0f);
}
CR_HD double fpu_visited_sqrt(int M) { return caro_sqrt((double)M * (1.0 / 4194304.0)); }
CR_HD double fpu_q_root(double base, double r, double s) {
  const double rs = r * s;
  return base - rs;
}
CR_HD float fpu_q(float base, double r, double s) {
  const double rs = r * s;
  return (float)((double)base - rs);
}

// The per-action piece of include/caro_hip.h ("virtual loss"), one statement for descend_level and caro_host_vl_level:
// the Q of an edge with n real visits, Q q0 as the level reads it (0 where n == 0) and vv > 0 virtual visits, all lost --
// the product, then the difference, then the quotient, in the level's precision (float64 at the root, float32 below it),
// the three counts converted from int.  No contraction, as above.
CR_HD double vl_q_root(double q0, int n, int vv) {
  const double w = q0 * (double)n;
  const double d = w - (double)vv;
  return d / (double)(n + vv);
}
CR_HD float vl_q(float q0, int n, int vv) {
  const float w = q0 * (float)n;
  const float d = w - (float)vv;
  return d / (float)(n + vv);
}

// The pieces of include/caro_hip.h ("temperature"), one statement for the ply (step_body), caro_policy (root_policy) and
// the host helper caro_host_temperature.  temp_early: is a ply with `step` searched plies behind it EARLY?  temp_move /
// temp_tuple: the ply's two temperatures.  temp_weight: w_a of a count n in a row whose maximum is nmax > 0, at a tau
// that is neither 0 nor 1 -- the quotient, the logarithm, the division by tau, the exponential, in float64.  No
// contraction, as above.  (The sum S of the weights is SEQUENTIAL in action order wherever it is formed.)
CR_HD bool temp_early(int step, int sbt0) { return sbt0 > 0 && step < sbt0; }
CR_HD double temp_move(bool early, double tau_early, double tau_late) { return early ? tau_early : tau_late; }
CR_HD double temp_tuple(double tau_m, int visit_targets) { return visit_targets ? 1.0 : tau_m; }
CR_HD double temp_weight(int n, int nmax, double tau) {
  if (n == 0) return 0.0;
  if (n == nmax) return 1.0;
  const double ratio = (double)n / (double)nmax;
  const double lg = caro_log(ratio);
  return caro_exp(lg / tau);
}
// a temperature the feature takes: 0 or in [0.05, 8] (a NaN fails every comparison)
CR_HD bool temp_valid(double tau) { return tau == 0.0 || (tau >= 0.05 && tau <= 8.0); }

// The pick rule of include/caro_hip.h ("position analysis"), one statement for k_lines and caro_host_line_heads: WHICH
// edge of a count row.  line_key orders the visited edges by (N descending, action ascending) as one integer -- a larger
// key ranks earlier, an edge without visits has key 0 and is never picked (a <= 255, n < 2^30).  line_pick is one step of
// "the largest key below `below`": folded over a row from best = 0 with below = LINE_KEY_TOP it gives the first maximum
// of N (np.argmax's rule), with below = the previous pick the next edge of the ranking; 0 = no such edge.  Integers only:
// the lanes of a wave fold their own actions and reduce with max in any order.
constexpr uint64_t LINE_KEY_TOP = ~0ULL;
CR_HD uint64_t line_key(int n, int a) { return n > 0 ? (((uint64_t)(uint32_t)n << 8) | (uint64_t)(255 - a)) : 0ULL; }
CR_HD uint64_t line_pick(uint64_t best, uint64_t key, uint64_t below) { return (key < below && key > best) ? key : best; }
CR_HD int line_key_action(uint64_t key) { return 255 - (int)(key & 255ULL); }

#define DISPATCH(var, EXPR)                                          \
  switch (var) {                                                     \
    case V_C4: { using GEO = GeoC4; EXPR; } break;                   \
    case V_M16: { using GEO = GeoM16; EXPR; } break;                 \
    case V_M32: { using GEO = GeoM32; EXPR; } break;                 \
    case V_M64: { using GEO = GeoM64; EXPR; } break;                 \
    case V_M128: { using GEO = GeoM128; EXPR; } break;               \
    case V_M256: { using GEO = GeoM256; EXPR; } break;               \
    case V_K16: { using GEO = GeoK16; EXPR; } break;                 \
    case V_K32: { using GEO = GeoK32; EXPR; } break;                 \
    case V_K64: { using GEO = GeoK64; EXPR; } break;                 \
    case V_K128: { using GEO = GeoK128; EXPR; } break;               \
    case V_K256: { using GEO = GeoK256; EXPR; } break;               \
    default: return fail(CARO_E_INVAL, "unsupported game geometry"); \
  }

}  // namespace caro

#endif
