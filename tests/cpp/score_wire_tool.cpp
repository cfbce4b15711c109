// score_wire_tool.cpp -- pronto_wire::error_metrics_t from the command line (tests/test_score_wire.py).
//   score_wire_tool hash          the type's 8-byte fingerprint, hex
//   score_wire_tool encode FILE   writes the encoding of a fixed message: utime = 123456789012, field i = (i + 1) * 0.125 - 1
//                                 (except percent_ddt = +inf: what the script publishes when the truth did not move)
//   score_wire_tool decode FILE   decodes FILE: prints the return value, then (if >= 0) utime and the ten doubles with %.17g
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pronto_amd/csrc/pronto_wire.hpp"

int main(int argc, char **argv)
{
  using pronto_wire::error_metrics_t;
  if (argc >= 2 && !strcmp(argv[1], "hash")) {
    printf("%016llx\n", (unsigned long long) error_metrics_t::fingerprint());
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "encode")) {
    error_metrics_t m;
    double v[10];
    for (int i = 0; i < 10; i++) v[i] = (i + 1) * 0.125 - 1.0;
    m.utime = 123456789012LL;
    for (int i = 0; i < 3; i++) { m.pos_error[i] = v[i]; m.rpy_error[i] = v[4 + i]; }
    m.pos_error_norm = v[3];
    m.distance_travelled = v[7];
    m.percent_ddt = INFINITY;
    m.time_elapsed = v[9];
    std::vector<uint8_t> buf;
    m.encode(buf);
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    fclose(f);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "decode")) {
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf(4096);
    buf.resize(fread(buf.data(), 1, buf.size(), f));
    fclose(f);
    error_metrics_t m;
    const int rc = m.decode(buf.data(), buf.size());
    printf("%d\n", rc);
    if (rc < 0) return 0;
    printf("%lld\n", (long long) m.utime);
    const double v[10] = { m.pos_error[0], m.pos_error[1], m.pos_error[2], m.pos_error_norm, m.rpy_error[0], m.rpy_error[1], m.rpy_error[2],
                           m.distance_travelled, m.percent_ddt, m.time_elapsed };
    for (int i = 0; i < 10; i++) printf("%.17g\n", v[i]);
    return 0;
  }
  fprintf(stderr, "usage: score_wire_tool hash | encode FILE | decode FILE\n");
  return 1;
}
