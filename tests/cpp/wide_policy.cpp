// wide_policy.cpp -- TEST-ONLY driver of wide_update_choice (pronto_amd/csrc/pb_policy.hpp), built by tests/test_wide_policy.py with plain
// g++.  Reads tests/cpp/policy_table.cpp's update queries from stdin,
//   update <mapping> <generic_update> <orient> <r_kind> <all_broadcast> <masked> <idx> ...
// and prints for each "wide <family> <list> <host_args>" and, for up to six rows, " narrow <family> <list> <host_args>" as update_choice
// answers.  With the argument "enum": the value of UPD_WIDE and of every older enumerator of UpdateFamily.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include POLICY_HEADER

using namespace pb;

int main(int argc, char **argv)
{
  if (argc > 1 && std::string(argv[1]) == "enum") {
    printf("%d | %d %d %d %d %d %d %d\n", (int) UPD_WIDE, (int) UPD_CT_COOP, (int) UPD_CT_QUAD, (int) UPD_LANE_LIST, (int) UPD_QUAD_LIST,
           (int) UPD_LANE_RT, (int) UPD_COOP_RT, (int) UPD_QUAD_RT);
    return 0;
  }
  static const char *const names[4] = { "lane15", "coop15", "coop21", "quad21" };
  std::string ln;
  while (std::getline(std::cin, ln)) {
    std::istringstream in(ln);
    std::string what, mapname;
    int generic = 0, orient = 0, rkind = 0, all_bc = 0, masked = 0, v, map = -1;
    in >> what >> mapname >> generic >> orient >> rkind >> all_bc >> masked;
    for (int i = 0; i < 4; i++)
      if (mapname == names[i]) map = i;
    std::vector<int> idx;
    while (in >> v) idx.push_back(v);
    if (what != "update" || map < 0 || idx.empty() || idx.size() > 9) {
      fprintf(stderr, "wide_policy: bad query '%s'\n", ln.c_str());
      return 2;
    }
    const int m = (int) idx.size();
    const UpdateChoice w = wide_update_choice((Mapping) map, generic != 0, m, idx.data(), orient != 0, rkind, all_bc != 0, masked != 0);
    printf("wide %d %d %d", (int) w.family, w.list, (int) w.host_args);
    if (m <= 6) {
      const UpdateChoice u = update_choice((Mapping) map, generic != 0, m, idx.data(), orient != 0, rkind, all_bc != 0, masked != 0);
      printf(" narrow %d %d %d", (int) u.family, u.list, (int) u.host_args);
    }
    printf("\n");
  }
  return 0;
}
