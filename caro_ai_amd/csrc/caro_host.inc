// caro_host.inc -- host-side single-state helpers of the C-ABI (include/caro_hip.h: caro_host_*, caro_key_words,
// caro_action_space, caro_obs_cells), instantiated from the same caro_rules.h / caro_noise.h as the kernels.
// Included INSIDE an extern "C" block by caro_engine.hip (hipcc) and by oracle/asan/host_tu.cpp (g++ with
// -fsanitize=address,undefined); the including file provides `static int fail(int code, const std::string& msg)`.
int caro_key_words(int kind, int n) { return variant_kw(pick_variant(kind, n)); }
int caro_action_space(int kind, int n) { return kind == CARO_GAME_CONNECT4 ? 7 : n * n; }
int caro_obs_cells(int kind, int n) { return kind == CARO_GAME_CONNECT4 ? 42 : n * n; }

// ---- host helpers (same rules header, host instantiation)
#define HOST_DISPATCH(var, EXPR) DISPATCH(var, EXPR)

int caro_host_initial(int kind, int n, int k, uint64_t* key) {
  const Variant var = pick_variant(kind, n);
  const GameParams gp = make_gp(kind, n, k);
  HOST_DISPATCH(var, { auto b = GEO::R::initial(gp); for (int i = 0; i < GEO::KW; ++i) key[i] = b.w[i]; });
  return 0;
}
int caro_host_move(int kind, int n, int k, uint64_t* key, int move, int player, int* won) {
  const Variant var = pick_variant(kind, n);
  const GameParams gp = make_gp(kind, n, k);
  if (player != 0 && player != 1) return fail(CARO_E_INVAL, "player must be 0 or 1");
  if (move < 0 || move >= gp.A) return fail(CARO_E_INVAL, "move out of range");
  HOST_DISPATCH(var, {
    typename GEO::R::Board b;
    for (int i = 0; i < GEO::KW; ++i) b.w[i] = key[i];
    if (kind == CARO_GAME_CONNECT4 && !GEO::R::legal(gp, b, move)) return fail(CARO_E_INVAL, "column is full");
    *won = GEO::R::move(gp, b, move, player) ? 1 : 0;
    for (int i = 0; i < GEO::KW; ++i) key[i] = b.w[i];
  });
  return 0;
}
int caro_host_legal(int kind, int n, int k, const uint64_t* key, uint8_t* legal) {
  const Variant var = pick_variant(kind, n);
  const GameParams gp = make_gp(kind, n, k);
  HOST_DISPATCH(var, {
    typename GEO::R::Board b;
    for (int i = 0; i < GEO::KW; ++i) b.w[i] = key[i];
    for (int a = 0; a < gp.A; ++a) legal[a] = GEO::R::legal(gp, b, a) ? 1 : 0;
  });
  return 0;
}
int caro_host_encode(int kind, int n, int k, const uint64_t* key, int who, float* planes) {
  const Variant var = pick_variant(kind, n);
  const GameParams gp = make_gp(kind, n, k);
  const int HW = gp.rows * gp.cols;
  HOST_DISPATCH(var, {
    typename GEO::R::Board b;
    for (int i = 0; i < GEO::KW; ++i) b.w[i] = key[i];
    for (int i = 0; i < 2 * HW; ++i) planes[i] = GEO::R::plane(gp, b, who, i / HW, i % HW);
  });
  return 0;
}
int caro_host_noise_row(uint64_t seed, uint64_t uid, uint32_t ply, uint32_t sim, int A, double alpha, double* out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  double tmp[256];
  caro_noise_row(seed, uid, ply, sim, A, alpha, out, tmp);
  return 0;
}
double caro_host_move_uniform(uint64_t seed, uint64_t uid, uint32_t ply) { return caro_move_uniform(seed, uid, ply); }
double caro_host_resign_uniform(uint64_t seed, uint64_t uid) { return caro_resign_uniform(seed, uid); }
double caro_host_cap_uniform(uint64_t seed, uint64_t uid, uint32_t ply) { return caro_cap_uniform(seed, uid, ply); }

double caro_host_open_uniform(uint64_t seed, uint64_t uid, uint32_t i) { return caro_open_uniform(seed, uid, i); }
// the limits of caro_engine_set_openings (0 = ok); shared with the engine and the batched kernel
static int openings_check(const GameParams& gp, int max_plies, const char* who) {
  if (max_plies < 0 || max_plies > 64) return fail(CARO_E_INVAL, std::string(who) + ": max_plies must be in [0, 64]");
  if (max_plies >= gp.rows * gp.cols) return fail(CARO_E_INVAL, std::string(who) + ": max_plies must be below the board's cell count");
  return 0;
}
int caro_host_opening(int kind, int n, int k, uint64_t seed, uint64_t uid, int first, int max_plies, uint64_t* key,
                      int* player, int* made) {
  const Variant var = pick_variant(kind, n);
  if (var == V_BAD) return fail(CARO_E_INVAL, "unsupported game geometry");
  const GameParams gp = make_gp(kind, n, k);
  if (!key || !player || !made) return fail(CARO_E_INVAL, "null argument");
  if (first != 0 && first != 1) return fail(CARO_E_INVAL, "first must be 0 or 1");
  if (int rc = openings_check(gp, max_plies, "caro_host_opening")) return rc;
  HOST_DISPATCH(var, {
    typename GEO::R::Board b;
    int p = first;
    *made = opening_position<typename GEO::R>(gp, seed, uid, max_plies, b, p);
    *player = p;
    for (int i = 0; i < GEO::KW; ++i) key[i] = b.w[i];
  });
  return 0;
}

// ---- forced playouts (include/caro_hip.h, "forced playouts"): the two rules on one row, from the functions the kernels call
static int forced_k_check(double k, const char* who) {
  if (!(k >= 0.0 && k <= 64.0)) return fail(CARO_E_INVAL, std::string(who) + ": k must be in [0, 64]");
  return 0;
}
int caro_host_forced_root(int A, const int32_t* N, const float* P, const double* noise, const uint8_t* legal,
                          double explore, double k, uint8_t* forced_out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  if (!N || !P || !noise || !legal || !forced_out) return fail(CARO_E_INVAL, "null argument");
  if (int rc = forced_k_check(k, "caro_host_forced_root")) return rc;
  long long T = 0;
  for (int a = 0; a < A; ++a) {
    if (N[a] < 0 || N[a] >= (1 << 30)) return fail(CARO_E_INVAL, "visit count out of range");
    T += N[a];
  }
  if (T >= (1ll << 30)) return fail(CARO_E_INVAL, "visit total out of range");
  const float keepf = (float)(1.0 - explore);
  int count = 0;
  for (int a = 0; a < A; ++a) {
    const float keep = keepf * P[a];
    const double prob = (double)keep + explore * noise[a];
    forced_out[a] = (legal[a] && fp_forced(N[a], (int)T, prob, k)) ? 1 : 0;
    count += forced_out[a];
  }
  return count;
}
int caro_host_forced_prune(int A, const int32_t* N, const double* Q, const float* P, float c_puct, double k,
                           int32_t* N_out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  if (!N || !Q || !P || !N_out) return fail(CARO_E_INVAL, "null argument");
  if (int rc = forced_k_check(k, "caro_host_forced_prune")) return rc;
  long long T = 0;
  int b = 0;
  for (int a = 0; a < A; ++a) {
    if (N[a] < 0 || N[a] >= (1 << 30)) return fail(CARO_E_INVAL, "visit count out of range");
    if (N[a] > N[b]) b = a;
    T += N[a];
  }
  if (T >= (1ll << 30)) return fail(CARO_E_INVAL, "visit total out of range");
  if (T == 0) return fail(CARO_E_INVAL, "caro_host_forced_prune: a row without visits has no policy (a refused ply)");
  const double sq = caro_sqrt((double)T), c = (double)c_puct;
  const double sstar = fp_score(Q[b], c, (double)P[b], sq, N[b]);
  for (int a = 0; a < A; ++a)
    N_out[a] = (a == b || N[a] == 0) ? N[a] : fp_pruned(N[a], Q[a], (double)P[a], c, k, (int)T, sq, sstar);
  return b;
}

// ---- first-play urgency (include/caro_hip.h, "first-play urgency"): one level of a descent on one row, with the scoring
// of descend_level restated for a single thread and the per-action pieces (fpu_mass, fpu_visited_sqrt, fpu_q_root, fpu_q)
// the kernels call.  reduction == 0: the level as an engine never told of the feature scores it.
static int fpu_reduction_check(double r, const char* who) {
  if (!(r >= 0.0 && r <= 2.0)) return fail(CARO_E_INVAL, std::string(who) + ": a reduction must be in [0, 2]");
  return 0;
}
int caro_host_fpu_level(int A, int root, const int32_t* N, const float* W, const float* Q, const float* P,
                        const int32_t* strong, const uint8_t* legal, const double* noise, float c_puct, double explore,
                        float q_up, double reduction, double* scores_out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  if (!N || !W || !Q || !P || !strong || !legal || !scores_out) return fail(CARO_E_INVAL, "null argument");
  if (root && !noise) return fail(CARO_E_INVAL, "caro_host_fpu_level: the root level needs a noise row");
  if (int rc = fpu_reduction_check(reduction, "caro_host_fpu_level")) return rc;
  long long T = 0;
  for (int a = 0; a < A; ++a) {
    if (N[a] < 0 || N[a] >= (1 << 24)) return fail(CARO_E_INVAL, "visit count out of range");
    T += N[a];
  }
  if (T >= (1ll << 24)) return fail(CARO_E_INVAL, "visit total out of range");
  const int nsum = (int)T;
  const bool fpu = reduction > 0.0;
  double s = 0.0;
  if (fpu) {
    int ms = 0;
    for (int a = 0; a < A; ++a)
      if (N[a] > 0 && legal[a]) ms += fpu_mass(P[a]);
    s = fpu_visited_sqrt(ms);
  }
  auto edge_qd = [&](int a) {  // the edge's Q as the root level reads it
    if (strong[a]) return (double)Q[a];
    return N[a] > 0 ? (double)W[a] / (double)N[a] : 0.0;
  };
  int choice = 0;
  if (root) {
    double qsub = 0.0;
    if (fpu) {
      int bn = 0;
      for (int a = 1; a < A; ++a)
        if (N[a] > N[bn]) bn = a;
      const double base = N[bn] > 0 ? edge_qd(bn) : 0.0;
      qsub = fpu_q_root(base, reduction, s);
    }
    const double sq = caro_sqrt((double)nsum);
    const double c64 = (double)c_puct;
    const float keepf = (float)(1.0 - explore);
    double best = -__builtin_huge_val();
    for (int a = 0; a < A; ++a) {
      const float keep = keepf * P[a];
      const double prob = (double)keep + explore * noise[a];
      const double u = ((c64 * prob) * sq) / (double)(1 + N[a]);
      double qd = edge_qd(a);
      if (fpu && N[a] == 0) qd = qsub;
      double sc = qd + u;
      if (!legal[a]) sc = -__builtin_huge_val();
      scores_out[a] = sc;
      if (sc > best) {
        best = sc;
        choice = a;
      }
    }
  } else {
    const float sqf = __builtin_sqrtf((float)nsum);  // (= sqrt_count of the kernels: IEEE correctly rounded)
    float qsubf = 0.0f;
    if (fpu) qsubf = fpu_q(-q_up, reduction, s);
    float bs = -__builtin_huge_valf();
    for (int a = 0; a < A; ++a) {
      float tt = c_puct * P[a];
      tt = tt * sqf;
      tt = tt / (float)(1 + N[a]);
      float qv = Q[a];
      if (fpu && N[a] == 0) qv = qsubf;
      float sc = qv + tt;
      if (!legal[a]) sc = -__builtin_huge_valf();
      scores_out[a] = (double)sc;
      if (sc > bs) {
        bs = sc;
        choice = a;
      }
    }
  }
  return choice;
}

// ---- virtual loss (include/caro_hip.h, "virtual loss"): one level of a descent on one row with the counts c of the rule
// given, the scoring of level_score restated for a single thread with the per-action pieces (vl_q_root, vl_q) the kernels
// call.  All c == 0 or n_vl == 0: the level as an engine never told of the feature scores it.
int caro_host_vl_level(int A, int root, const int32_t* N, const float* W, const float* Q, const float* P,
                       const int32_t* strong, const uint8_t* legal, const double* noise, float c_puct, double explore,
                       const int32_t* c, int n_vl, double* scores_out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  if (!N || !W || !Q || !P || !strong || !legal || !c || !scores_out) return fail(CARO_E_INVAL, "null argument");
  if (root && !noise) return fail(CARO_E_INVAL, "caro_host_vl_level: the root level needs a noise row");
  if (n_vl < 0 || n_vl > 16) return fail(CARO_E_INVAL, "caro_host_vl_level: n_vl must be in [0, 16]");
  long long T = 0;
  for (int a = 0; a < A; ++a) {
    if (N[a] < 0 || N[a] >= (1 << 24)) return fail(CARO_E_INVAL, "visit count out of range");
    if (c[a] < 0 || c[a] > 64) return fail(CARO_E_INVAL, "caro_host_vl_level: a count must be in [0, 64]");
    T += N[a] + n_vl * c[a];
  }
  if (T >= (1ll << 24)) return fail(CARO_E_INVAL, "visit total out of range");
  const int nsum = (int)T;  // nsum'
  int choice = 0;
  if (root) {
    const double sq = caro_sqrt((double)nsum);
    const double c64 = (double)c_puct;
    const float keepf = (float)(1.0 - explore);
    double best = -__builtin_huge_val();
    for (int a = 0; a < A; ++a) {
      const int vv = n_vl * c[a], n1 = N[a] + vv;
      const float keep = keepf * P[a];
      const double prob = (double)keep + explore * noise[a];
      const double u = ((c64 * prob) * sq) / (double)(1 + n1);
      double qd;
      if (strong[a]) qd = (double)Q[a];
      else qd = N[a] > 0 ? (double)W[a] / (double)N[a] : 0.0;
      if (vv > 0) qd = vl_q_root(N[a] > 0 ? qd : 0.0, N[a], vv);
      double sc = qd + u;
      if (!legal[a]) sc = -__builtin_huge_val();
      scores_out[a] = sc;
      if (sc > best) {
        best = sc;
        choice = a;
      }
    }
  } else {
    const float sqf = __builtin_sqrtf((float)nsum);  // (= sqrt_count of the kernels: IEEE correctly rounded)
    float bs = -__builtin_huge_valf();
    for (int a = 0; a < A; ++a) {
      const int vv = n_vl * c[a], n1 = N[a] + vv;
      float tt = c_puct * P[a];
      tt = tt * sqf;
      tt = tt / (float)(1 + n1);
      float qv = Q[a];
      if (vv > 0) qv = vl_q(N[a] > 0 ? qv : 0.0f, N[a], vv);
      float sc = qv + tt;
      if (!legal[a]) sc = -__builtin_huge_valf();
      scores_out[a] = (double)sc;
      if (sc > bs) {
        bs = sc;
        choice = a;
      }
    }
  }
  return choice;
}

// ---- temperature (include/caro_hip.h, "temperature"): T(N, tau) of one count row, from the functions the kernels call
// (temp_weight; the sum of the weights sequential in action order, as the ply forms it).
static int temp_tau_check(double tau, const char* who) {
  if (!temp_valid(tau)) return fail(CARO_E_INVAL, std::string(who) + ": a temperature must be 0 or in [0.05, 8]");
  return 0;
}
int caro_host_temperature(int A, const int32_t* N, double tau, double* pi_out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  if (!N || !pi_out) return fail(CARO_E_INVAL, "null argument");
  if (int rc = temp_tau_check(tau, "caro_host_temperature")) return rc;
  long long T = 0;
  int b = 0;
  for (int a = 0; a < A; ++a) {
    if (N[a] < 0 || N[a] >= (1 << 30)) return fail(CARO_E_INVAL, "visit count out of range");
    if (N[a] > N[b]) b = a;
    T += N[a];
  }
  if (T >= (1ll << 30)) return fail(CARO_E_INVAL, "visit total out of range");
  if (T == 0 && tau > 0.0) return fail(CARO_E_INVAL, "caro_host_temperature: a row without visits has no policy at tau > 0 (a refused ply)");
  if (tau == 0.0) {
    for (int a = 0; a < A; ++a) pi_out[a] = a == b ? 1.0 : 0.0;
  } else if (tau == 1.0) {
    for (int a = 0; a < A; ++a) pi_out[a] = (double)N[a] / (double)T;
  } else {
    double S = 0.0;
    for (int a = 0; a < A; ++a) {
      pi_out[a] = temp_weight(N[a], N[b], tau);
      S = S + pi_out[a];
    }
    for (int a = 0; a < A; ++a) pi_out[a] = pi_out[a] / S;
  }
  return b;
}

// ---- position analysis (include/caro_hip.h, "position analysis"): the heads of the lines of one root row, from the
// functions k_lines calls (line_key / line_pick: rank by N descending, action ascending; heads_out[0] is the first maximum).
int caro_host_line_heads(int A, const int32_t* N, int top, int32_t* heads_out) {
  if (A < 1 || A > 256) return fail(CARO_E_INVAL, "A out of range");
  if (!N || !heads_out) return fail(CARO_E_INVAL, "null argument");
  if (top < 1 || top > 16) return fail(CARO_E_INVAL, "caro_host_line_heads: top must be in [1, 16]");
  for (int a = 0; a < A; ++a)
    if (N[a] < 0 || N[a] >= (1 << 30)) return fail(CARO_E_INVAL, "visit count out of range");
  int n_lines = 0;
  uint64_t below = LINE_KEY_TOP;
  for (int j = 0; j < top; ++j) {
    uint64_t best = 0;
    for (int a = 0; a < A; ++a) best = line_pick(best, line_key(N[a], a), below);
    heads_out[j] = best ? line_key_action(best) : -1;
    if (best) ++n_lines;
    below = best;  // (0 once the row is exhausted: nothing is below it)
  }
  return n_lines;
}
