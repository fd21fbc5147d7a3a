// trajectory_check.cpp -- csrc/vh_trajectory.h compiled for the host: one chain of rows walked with the header's own
// functions, the records written as vh_trajectory writes them (tests/test_trajectory.py).
//   in : int32 on_fail, int32 n, double T0[16], then n x { double tr[6] }, then n x int32 ok
//   out: n x vh_traj_pose, then one vh_traj_carry
#include "../../hls-final-visual-odometry_amd/csrc/vh_trajectory.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t on_fail = 0, n = 0;
  vh_traj_carry c;
  memset(&c, 0, sizeof c);
  if (fread(&on_fail, 4, 1, fi) != 1 || fread(&n, 4, 1, fi) != 1 || n < 0 || fread(c.Tw, 8, 16, fi) != 16) return 2;
  std::vector<double> tr(6 * (size_t)n + 1);
  std::vector<int32_t> ok((size_t)n + 1);
  if (fread(tr.data(), 8, 6 * (size_t)n, fi) != 6 * (size_t)n || fread(ok.data(), 4, (size_t)n, fi) != (size_t)n) return 2;
  fclose(fi);
  std::vector<vh_traj_pose> out((size_t)n);
  for (int32_t r = 0; r < n; r++) {
    vh_traj_pose &o = out[(size_t)r];
    memset(&o, 0, sizeof o);
    double Tinv[16];
    o.status = traj_inverse(&tr[6 * (size_t)r], ok[(size_t)r], Tinv);
    const int32_t act = traj_action(o.status, on_fail, c.has_tinv);
    if (act == 1) { memcpy(c.Tinv, Tinv, sizeof Tinv); c.has_tinv = 1; c.step++; }
    memcpy(o.Tw_prev, c.Tw, sizeof c.Tw);
    if (act) {
      double P[16];
      for (int32_t i = 0; i < 4; i++)
        for (int32_t j = 0; j < 4; j++) {
          const double mcol[4] = {c.Tinv[j], c.Tinv[4 + j], c.Tinv[8 + j], c.Tinv[12 + j]};
          P[4 * i + j] = traj_dot(&c.Tw[4 * i], mcol);
        }
      memcpy(c.Tw, P, sizeof P);
    }
    memcpy(o.Tw_cur, c.Tw, sizeof c.Tw);
    o.step = c.step;
  }
  FILE *fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  fwrite(out.data(), sizeof(vh_traj_pose), (size_t)n, fo);
  fwrite(&c, sizeof c, 1, fo);
  fclose(fo);
  return 0;
}
