// flow_wire_tool.cpp -- pronto::optical_flow_t of pronto_amd/csrc/pronto_wire.hpp for tests/test_flow_wire.py:
//   hash          the type's fingerprint, hex
//   encode        the wire image, hex, of the message with utime = 1234567890123 and field k (in the .lcm file's order) = (k + 1) / 8 - 0.3
//   decode HEX    the fields of a wire image, one per line as hex floats in the STRUCT's named order; or "error N"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../pronto_amd/csrc/pronto_wire.hpp"

using namespace pronto_wire;

int main(int argc, char **argv)
{
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "hash")) {
    printf("%016llx\n", (unsigned long long) optical_flow_t::fingerprint());
    return 0;
  }
  if (!strcmp(argv[1], "encode")) {
    optical_flow_t m;
    m.utime = 1234567890123LL;
    double *f[10] = { &m.dt, &m.ux, &m.uy, &m.scale, &m.theta, &m.alpha1, &m.alpha2, &m.gamma, &m.conf_rs, &m.conf_xy };
    for (int k = 0; k < 10; k++) *f[k] = (k + 1) / 8.0 - 0.3;
    std::vector<uint8_t> out;
    m.encode(out);
    for (uint8_t b : out) printf("%02x", b);
    printf("\n");
    return 0;
  }
  if (!strcmp(argv[1], "decode") && argc > 2) {
    std::vector<uint8_t> in;
    const std::string hex = argv[2];
    for (size_t i = 0; i + 1 < hex.size(); i += 2) in.push_back((uint8_t) std::stoi(hex.substr(i, 2), nullptr, 16));
    optical_flow_t m;
    const int rc = m.decode(in.data(), in.size());
    if (rc < 0) {
      printf("error %d\n", rc);
      return 0;
    }
    printf("used %d\nutime %lld\nux %a\nuy %a\ntheta %a\nscale %a\nalpha1 %a\nalpha2 %a\ngamma %a\ndt %a\nconf_rs %a\nconf_xy %a\n", rc, (long long) m.utime,
           m.ux, m.uy, m.theta, m.scale, m.alpha1, m.alpha2, m.gamma, m.dt, m.conf_rs, m.conf_xy);
    return 0;
  }
  return 2;
}
