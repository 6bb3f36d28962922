// Which instantiation of the one-pass walk a launch takes: the laboratory switches read into TileKnobs, and the rule that turns
// precision, arithmetic and knobs into a TileRoute.  Host only and free of HIP headers (tests/native/tile_route_check.cpp compiles
// it with plain g++).  Internal.
#pragma once
#include <cstring>

#include "env.h"

namespace nbody {

// Which instantiation launch_tree_walk_tile_main launched (the NBODY_TRACE route line): the arm ("exact": walk_tile<T, false>,
// "fast-registers": walk_tile_fast, "fast-rows": walk_tile<T, true>; laboratory only: "fast-bfs", "fast-registers-log"), and
// the template parameters that arm has: the LDS tile's rows and whether node records come by scalar loads (exact, fast-rows),
// the node-record mode (fast-registers).  -1: that arm has no such parameter.
struct TileRoute {
  const char* arm = "none";
  int rows = -1, srec = -1, rec_mode = -1;
};
inline bool arm_is(const TileRoute& r, const char* arm) { return std::strcmp(r.arm, arm) == 0; }

// The laboratory switches of the one-pass walk; the defaults are the product's values (and all the product build ever sees).
struct TileKnobs {
  // rows of the LDS tile: 8 keep it at 4 KB per wave, eight waves per SIMD (NBODY_WALK_TILE_TARGETS: 4 / 16)
  int rows = 8;
  // node records by scalar loads (scalar_node_rec): the exact walk always (62 instead of 72 VGPRs: eight waves per SIMD instead of seven;
  // reference scene 0.579 -> 0.567 ms, Plummer 1 M 6.07 -> 5.96); NBODY_WALK_SCALAR_REC=0: the vector loads of one address
  bool srec = true;
  // FAST: f32 takes walk_tile_fast (registers, lane-parallel sums); f64 the rows arm (walk_tile<double, true>: LDS rows + ordered adds with
  // the one-reciprocal term) — walk_tile_fast<double> moves every value as two 32-bit halves through the swaps and runs at half
  // the occupancy: Plummer 4 M f64 205 ms against 92 (the exact walk: 124).  -1: by precision; NBODY_WALK_FAST_ROWS=0/1 forces one or the other.
  int fast_rows = -1;
  // FAST: node records by scalar loads (round 3 took vector loads of one address below 400 000 targets: 0.298 against 0.322 ms on the
  // reference scene's FIRST steps; over the bench leg's 300 steps, with the waves in one residency round, scalar loads win there too:
  // 0.299 -> 0.277 ms, profiles/r04_walk_wave_target.txt).  NBODY_WALK_FAST_REC=0 / 1: the plain / pinned vector loads.
  int rec_mode = 3;
  bool wave_log = false;  // NBODY_WALK_WAVE_LOG=1 (development): per-wave time and step counts of the FAST register walk
  // NBODY_WALK_FAST_BFS=1: round 4's breadth-first FAST walk (walk_tile_fast_bfs) — measured SLOWER than the depth-first kernel
  // (reference scene 0.579 against 0.338 ms, Plummer 1 M 4.96 against 2.99: profiles/r04_walk_bfs_ab.txt), kept for that A/B only
  bool bfs = false;
};

// Read at every launch, never latched: a test that switches variants inside one process would otherwise compare one kernel with
// itself.  Through lab_int: the product build returns the defaults whatever the environment holds.
inline TileKnobs tile_knobs_from_env() {
  TileKnobs k;
  k.rows = lab_int("NBODY_WALK_TILE_TARGETS", k.rows);
  k.srec = lab_int("NBODY_WALK_SCALAR_REC", 1) != 0;
  k.fast_rows = lab_int("NBODY_WALK_FAST_ROWS", k.fast_rows);
  const int rec = lab_int("NBODY_WALK_FAST_REC", -1);
  k.rec_mode = rec >= 0 ? rec : k.rec_mode;
  k.wave_log = lab_int("NBODY_WALK_WAVE_LOG", 0) != 0;
  k.bfs = lab_int("NBODY_WALK_FAST_BFS", 0) != 0;
  return k;
}

// The one rule.  Exact arithmetic walks the rows arm.  FAST walks the rows arm where fast_rows says so (by precision: f64), else
// the registers: breadth first if asked for (f32 only, and not while the per-wave log is on), else depth first, where the log
// has one kernel of its own (node records by plain loads) and a record mode other than 1 or 3 reads as 0.  A row count other
// than 4 or 16 reads as 8.
inline TileRoute choose_tile_route(bool f64, bool fast, const TileKnobs& k) {
  const bool fast_rows = k.fast_rows >= 0 ? k.fast_rows != 0 : f64;
  if (fast && !fast_rows) {
    const bool log = k.wave_log;
    if (!f64 && !log && k.bfs) return TileRoute{"fast-bfs", -1, -1, -1};
    if (log) return TileRoute{"fast-registers-log", -1, -1, 0};
    return TileRoute{"fast-registers", -1, -1, (k.rec_mode == 1 || k.rec_mode == 3) ? k.rec_mode : 0};
  }
  const int rows = (k.rows == 16 || k.rows == 4) ? k.rows : 8;
  return TileRoute{fast ? "fast-rows" : "exact", rows, k.srec ? 1 : 0, -1};
}

}  // namespace nbody
