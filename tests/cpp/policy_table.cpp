// policy_table.cpp -- prints what pronto_amd/csrc/pb_policy.hpp decides, on the CPU (tests/test_kernel_policy.py; no HIP, no library).
//   policy_table contexts   the policy of a context for the built-in table of (state size, batch, switches): the switches are put into
//                           this process's environment and read back through read_switches(), one line per context
//   policy_table names      pb_hot_kernel's twelve names
//   policy_table hints      the cache policy of the kernels built for two of the three, for MH = 0, 1, 2
//   policy_table query      answers the questions on standard input, one per line:
//                             update <mapping> <generic_update> <orient> <r_kind> <all_broadcast> <masked> <idx> ...
//                             args <mapping> <corr_kind>            pb_step_legodo_correct's argument form
//                             pair <mapping> <world_constraint> <mode>
//                             replay <mapping> <onelane> <write_through>
//                             smooth <mapping> <ntiles> <n_cu>      (switches from the environment)
//                           <mapping>: lane15, coop15, coop21, quad21
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include POLICY_HEADER

using namespace pb;

typedef std::vector<std::pair<const char *, const char *>> Env;   // names without the PRONTO_ prefix

static const char *const kSwitches[] = { "BATCH_COOP15", "BATCH_HALF", "BATCH_REPLAY_ONELANE", "BATCH_XCD", "BATCH_GENERIC_UPDATE", "BATCH_QUAD21",
                                         "BATCH_MEMHINT", "BATCH_BLOCKED", "BATCH_BLOCK_FILTERS", "SMOOTH_KERNEL", "SMOOTH_PIVOT", "SMOOTH_GRID" };

static void set_env(const Env &env)
{
  for (const char *s : kSwitches) unsetenv((std::string("PRONTO_") + s).c_str());
  for (const auto &e : env) setenv((std::string("PRONTO_") + e.first).c_str(), e.second, 1);
}

static const char *const kMapName[] = { "lane15", "coop15", "coop21", "quad21" };
static const char *const kSmoothName[] = { "k_smooth_wide<15>", "k_smooth_lane", "k_smooth_reg<false>", "k_smooth_reg<true>" };
static const char *const kReplayName[] = { "k_replay_fused<15>", "k_replay_coop<15>", "k_replay_coop<21>", "k_replay_quad<1>" };

// one context: what pb_create keeps and what its launchers make of it
static void describe_context(int ns, long batch)
{
  const Policy p = make_policy(ns, batch, state_bytes(ns, batch), read_switches());
  printf("step=%s half=%d xcd=%d generic=%d onelane=%d run_block=%d", step_kernel_name(p.step.map, p.mem_hint), (int) p.step.half, (int) p.xcd_remap,
         (int) p.generic_update, (int) p.replay_onelane, p.run_block);
  if (p.run_block > 0) printf(" block_step=%s", step_kernel_name(p.run_block_map, p.run_block_hint));
  const int ntiles = (int) ((batch + 63) / 64);
  printf(" smooth=%s wide_grid=%d\n", kSmoothName[smooth_kernel(p)], smooth_wide_grid(p, ntiles, 256));
}

static void contexts()
{
  // both sides of: 393 216 filters (coop15); 48 / 310 / 350 MB of state (cache policy; 350 MB is exactly 327 680 15-state filters);
  // 256 MB (blocked order); the block sizes 229 376 / 114 688; uneven block counts; batches that are no multiple of 64; 1 and 64
  static const long batches[] = { 1, 64, 100, 130, 4096, 24384, 24448, 32768, 44928, 44992, 65536, 114688, 114752, 130048, 130112, 131072, 157440,
                                  157504, 177792, 177856, 229376, 229440, 239616, 239680, 262144, 290176, 290240, 327616, 327680, 344064, 393216,
                                  393217, 393280, 458752, 458816, 524288, 1000000, 1048576 };
  static const long few[] = { 64, 65536, 131072, 393280, 524288 };
  // with every batch
  static const Env narrow[] = { {}, { { "BATCH_BLOCKED", "1" } }, { { "BATCH_COOP15", "1" }, { "BATCH_BLOCKED", "1" } },
                                { { "BATCH_MEMHINT", "2" }, { "BATCH_BLOCKED", "1" } }, { { "BATCH_COOP15", "0" }, { "BATCH_BLOCKED", "0" } } };
  // every switch at each documented value and at values outside them; the combinations the GPU tests run
  static const Env wide[] = {
    { { "BATCH_COOP15", "0" } }, { { "BATCH_COOP15", "1" } }, { { "BATCH_COOP15", "" } }, { { "BATCH_HALF", "1" } }, { { "BATCH_HALF", "0" } },
    { { "BATCH_HALF", "1" }, { "BATCH_COOP15", "0" } }, { { "BATCH_HALF", "1" }, { "BATCH_COOP15", "1" } }, { { "BATCH_REPLAY_ONELANE", "1" } },
    { { "BATCH_REPLAY_ONELANE", "0" } }, { { "BATCH_XCD", "0" } }, { { "BATCH_XCD", "1" } }, { { "BATCH_GENERIC_UPDATE", "1" } },
    { { "BATCH_GENERIC_UPDATE", "0" } }, { { "BATCH_QUAD21", "0" } }, { { "BATCH_QUAD21", "1" } }, { { "BATCH_MEMHINT", "0" } },
    { { "BATCH_MEMHINT", "1" } }, { { "BATCH_MEMHINT", "2" } }, { { "BATCH_MEMHINT", "3" } }, { { "BATCH_MEMHINT", "-1" } }, { { "BATCH_MEMHINT", "" } },
    { { "BATCH_BLOCKED", "0" } }, { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "32768" } },
    { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "1000" } }, { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "0" } },
    { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "44928" } }, { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "44992" } },
    { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "24384" } }, { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "24448" } },
    { { "BATCH_BLOCK_FILTERS", "16384" } }, { { "BATCH_COOP15", "0" }, { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "16384" } },
    { { "BATCH_COOP15", "1" }, { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "16384" }, { "BATCH_MEMHINT", "1" } },
    { { "BATCH_COOP15", "1" }, { "BATCH_MEMHINT", "2" } }, { { "BATCH_QUAD21", "0" }, { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", "16384" } },
    { { "SMOOTH_KERNEL", "lane" } }, { { "SMOOTH_KERNEL", "reg" } }, { { "SMOOTH_KERNEL", "wide" } }, { { "SMOOTH_PIVOT", "1" } },
    { { "SMOOTH_PIVOT", "0" } }, { { "SMOOTH_PIVOT", "1" }, { "SMOOTH_KERNEL", "lane" } }, { { "SMOOTH_GRID", "64" } }, { { "SMOOTH_GRID", "2048" } },
    { { "SMOOTH_GRID", "0" } }, { { "SMOOTH_GRID", "-4" } },
  };
  auto line = [](int ns, long batch, const Env &env) {
    set_env(env);
    printf("n=%d batch=%ld", ns, batch);
    for (const auto &e : env) printf(" %s=%s", e.first, e.second);
    printf(" -> ");
    describe_context(ns, batch);
  };
  // two blocks of exactly the sizes on both sides of the per-block 48 MB (15 states: 44 928 / 44 992 filters, 21: 24 384 / 24 448)
  static const long edge_blocks[] = { 44928, 44992, 24384, 24448 };
  for (int ns : { 15, 21 }) {
    for (long b : batches)
      for (const Env &env : narrow) line(ns, b, env);
    for (long b : few)
      for (const Env &env : wide) line(ns, b, env);
    for (long blk : edge_blocks) {
      const std::string filters = std::to_string(blk);
      line(ns, 2 * blk, { { "BATCH_BLOCKED", "1" }, { "BATCH_BLOCK_FILTERS", filters.c_str() } });
    }
  }
}

static const char *const kCorrName[] = { "CorrVel", "CorrPos", "CorrPosVel", "CorrPosOrient", "CorrPosYaw", "CorrVelYaw", "CorrYaw", "CorrGpfYawPos",
                                         "CorrGpfChiPos", "CorrGpfZ" };

// the kernel of an update choice, in the notation of tests/test_update_ill_conditioned.py's table
static std::string update_kernel_name(const UpdateChoice &u, int ns, int m, bool orient)
{
  char b[96];
  switch (u.family) {
  case UPD_CT_COOP: snprintf(b, sizeof b, "k_step_coop<%d,false,.,%s>", ns, kCorrName[u.list]); break;
  case UPD_CT_QUAD: snprintf(b, sizeof b, "k_update_quad<%s>", kCorrName[u.list]); break;
  case UPD_LANE_LIST: snprintf(b, sizeof b, "k_update_lane<15,6,IdxVelOmega>"); break;
  case UPD_QUAD_LIST: snprintf(b, sizeof b, "k_update_quad_list<.,3,4,5,0,1,2>"); break;
  case UPD_LANE_RT: snprintf(b, sizeof b, "k_update_lane_rt<15,%d,%s>", m, orient ? "true" : "false"); break;
  case UPD_COOP_RT: snprintf(b, sizeof b, "k_update_coop_rt<%d>", m); break;
  case UPD_QUAD_RT: snprintf(b, sizeof b, "k_update_quad_rt<%d>", m); break;
  default: snprintf(b, sizeof b, "?"); break;
  }
  return b;
}

static bool mapping_of(const std::string &s, Mapping &map)
{
  for (int i = 0; i < 4; i++)
    if (s == kMapName[i]) {
      map = (Mapping) i;
      return true;
    }
  return false;
}

static int query()
{
  std::string ln;
  while (std::getline(std::cin, ln)) {
    std::istringstream in(ln);
    std::string what, mapname;
    Mapping map;
    if (!(in >> what >> mapname) || !mapping_of(mapname, map)) {
      fprintf(stderr, "policy_table: bad query '%s'\n", ln.c_str());
      return 2;
    }
    if (what == "update") {
      int generic = 0, orient = 0, rkind = 0, all_bc = 0, masked = 0, v;
      in >> generic >> orient >> rkind >> all_bc >> masked;
      std::vector<int> idx;
      while (in >> v) idx.push_back(v);
      if (idx.empty() || idx.size() > 6) return 2;
      const UpdateChoice u = update_choice(map, generic != 0, (int) idx.size(), idx.data(), orient != 0, rkind, all_bc != 0, masked != 0);
      printf("%s host_args=%d\n", update_kernel_name(u, mapping_states(map), (int) idx.size(), orient != 0).c_str(), (int) u.host_args);
    } else if (what == "args") {
      int kind = 0;
      in >> kind;
      printf("%d\n", (int) correction_as_args(map, kind));
    } else if (what == "pair") {
      int wc = 0, mode = 0;
      in >> wc >> mode;
      printf("%d\n", (int) pair_kernel_exists(map, wc != 0, mode));
    } else if (what == "replay") {
      int onelane = 0, wt = 0;
      in >> onelane >> wt;
      Policy p;
      p.step.map = map;
      p.replay_onelane = onelane != 0;
      printf("%s\n", kReplayName[replay_kernel(p, wt != 0)]);
    } else if (what == "smooth") {
      int ntiles = 0, n_cu = 0;
      in >> ntiles >> n_cu;
      Policy p = make_policy(mapping_states(map), 64L * ntiles, state_bytes(mapping_states(map), 64L * ntiles), read_switches());
      printf("%s %d\n", kSmoothName[smooth_kernel(p)], smooth_wide_grid(p, ntiles, n_cu));
    } else {
      return 2;
    }
  }
  return 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "contexts") contexts();
  else if (mode == "names") {
    for (int map = 0; map < 4; map++)
      for (int mh = 0; mh < 3; mh++) printf("%s %d %s\n", kMapName[map], mh, step_kernel_name((Mapping) map, mh));
  } else if (mode == "hints") printf("%d %d %d\n", two_policy_hint(MH_DEFAULT), two_policy_hint(MH_STORE_SC1), two_policy_hint(MH_STREAM_NT));
  else if (mode == "query") return query();
  else {
    fprintf(stderr, "usage: policy_table contexts | names | hints | query\n");
    return 2;
  }
  return 0;
}
