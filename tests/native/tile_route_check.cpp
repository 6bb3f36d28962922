// csrc/walk_route.h on the CPU: choose_tile_route against a table of its own over every combination of precision, arithmetic and
// laboratory knobs, the four routes the product's defaults give, and (built without NBODY_LAB, as here) that the product's knobs are
// the defaults whatever the environment holds.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../nbody-simulation_amd/csrc/walk_route.h"

using nbody::TileKnobs;
using nbody::TileRoute;

namespace {

struct Want {
  std::string arm;
  int rows, srec, rec_mode;
};

// The rule as a table.  Arithmetic exact: the rows arm, whatever the FAST knobs say.  FAST: rows or registers by fast_rows (-1: f64
// rows, f32 registers); the register arm's variant by (log, bfs, precision).
Want expected(bool f64, bool fast, int rows, bool srec, int fast_rows, int rec_mode, bool log, bool bfs) {
  static const int kRowsOf[17] = {8, 8, 8, 8, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16};
  static const int kRecOf[4] = {0, 1, 0, 3};
  const int r = rows >= 0 && rows <= 16 ? kRowsOf[rows] : 8;
  if (!fast) return Want{"exact", r, srec ? 1 : 0, -1};
  const bool through_rows = fast_rows == 1 || (fast_rows == -1 && f64);
  if (through_rows) return Want{"fast-rows", r, srec ? 1 : 0, -1};
  // registers:      log  bfs  f64
  static const char* const kArm[2][2][2] = {{{"fast-registers", "fast-registers"}, {"fast-bfs", "fast-registers"}},
                                            {{"fast-registers-log", "fast-registers-log"}, {"fast-registers-log", "fast-registers-log"}}};
  const std::string arm = kArm[log][bfs][f64];
  if (arm == "fast-bfs") return Want{arm, -1, -1, -1};
  if (arm == "fast-registers-log") return Want{arm, -1, -1, 0};
  return Want{arm, -1, -1, kRecOf[rec_mode]};
}

int failures = 0;
void check(const TileRoute& got, const Want& want, const char* what) {
  if (want.arm != got.arm || want.rows != got.rows || want.srec != got.srec || want.rec_mode != got.rec_mode) {
    std::printf("MISMATCH %s: got %s %d %d %d, want %s %d %d %d\n", what, got.arm, got.rows, got.srec, got.rec_mode, want.arm.c_str(),
                want.rows, want.srec, want.rec_mode);
    ++failures;
  }
}

}  // namespace

int main() {
  int cases = 0;
  const int rows_of[4] = {4, 8, 16, 7}, fast_rows_of[3] = {-1, 0, 1};
  for (int f64 = 0; f64 < 2; ++f64)
    for (int fast = 0; fast < 2; ++fast)
      for (int rows : rows_of)
        for (int srec = 0; srec < 2; ++srec)
          for (int fast_rows : fast_rows_of)
            for (int rec_mode = 0; rec_mode < 4; ++rec_mode)
              for (int log = 0; log < 2; ++log)
                for (int bfs = 0; bfs < 2; ++bfs) {
                  TileKnobs k;
                  k.rows = rows;
                  k.srec = srec != 0;
                  k.fast_rows = fast_rows;
                  k.rec_mode = rec_mode;
                  k.wave_log = log != 0;
                  k.bfs = bfs != 0;
                  char what[96];
                  std::snprintf(what, sizeof what, "f64=%d fast=%d rows=%d srec=%d fast_rows=%d rec=%d log=%d bfs=%d", f64, fast, rows, srec,
                                fast_rows, rec_mode, log, bfs);
                  check(nbody::choose_tile_route(f64 != 0, fast != 0, k), expected(f64, fast, rows, srec, fast_rows, rec_mode, log, bfs), what);
                  ++cases;
                }
  // the product: default knobs (what tile_knobs_from_env returns in a build without NBODY_LAB, whatever the environment holds)
  const TileKnobs d;
  if (!(d.rows == 8 && d.srec && d.fast_rows == -1 && d.rec_mode == 3 && !d.wave_log && !d.bfs)) {
    std::printf("MISMATCH default knobs\n");
    ++failures;
  }
  check(nbody::choose_tile_route(false, false, d), Want{"exact", 8, 1, -1}, "product f32 exact");
  check(nbody::choose_tile_route(false, true, d), Want{"fast-registers", -1, -1, 3}, "product f32 FAST");
  check(nbody::choose_tile_route(true, false, d), Want{"exact", 8, 1, -1}, "product f64 exact");
  check(nbody::choose_tile_route(true, true, d), Want{"fast-rows", 8, 1, -1}, "product f64 FAST");
#ifndef NBODY_LAB
  setenv("NBODY_WALK_TILE_TARGETS", "16", 1);
  setenv("NBODY_WALK_SCALAR_REC", "0", 1);
  setenv("NBODY_WALK_FAST_ROWS", "1", 1);
  setenv("NBODY_WALK_FAST_REC", "1", 1);
  setenv("NBODY_WALK_WAVE_LOG", "1", 1);
  setenv("NBODY_WALK_FAST_BFS", "1", 1);
  const TileKnobs e = nbody::tile_knobs_from_env();
  if (!(e.rows == 8 && e.srec && e.fast_rows == -1 && e.rec_mode == 3 && !e.wave_log && !e.bfs)) {
    std::printf("MISMATCH the product build read a laboratory switch\n");
    ++failures;
  }
#endif
  if (cases != 2 * 2 * 4 * 2 * 3 * 4 * 2 * 2) {
    std::printf("MISMATCH %d cases\n", cases);
    ++failures;
  }
  if (failures) return 1;
  std::printf("OK %d combinations\n", cases);
  return 0;
}
