// The host's reader of state images and deltas (vigor_amd/csrc/vp_state_img.h)
// alone, for a build with the host compiler's sanitizers
// (tests/test_state_reader.py): the header's and every table's checks over a
// file, as vp_state_load and vp_state_delta_apply run them before anything is
// uploaded.
//
//   state_reader_main FILE image|delta nat|bridge|lb|fw|pol CAP [CAP2] [--truncations]
//
// Prints "rc text" (0, or -22 and the refusal). --truncations: one such line
// per length 0 .. size for the file's first bytes, each in a heap buffer of
// exactly that length, so that a read past the end is a sanitizer's report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../vigor_amd/csrc/vp_state_img.h"

using namespace vp::stimg;

static int check(const Format &f, const Expect &x, const uint8_t *buf, uint64_t bytes, char *msg,
                 size_t len) {
  int64_t last_now;
  Section sec[2];
  msg[0] = 0;
  if (!read_header(f, x, buf, bytes, &last_now, msg, len)) return -22;
  return read_sections(f, x, buf, bytes, sec, msg, len) ? 0 : -22;
}

int main(int argc, char **argv) {
  static const struct { const char *name; Expect x; } kinds[] = {
      {"nat", {1, 1, {}, {TT_NAT}}},        {"bridge", {2, 1, {}, {TT_BRIDGE}}},
      {"lb", {3, 2, {}, {TT_LBFLOW, TT_LBBACK}}}, {"fw", {4, 1, {}, {TT_FW}}},
      {"pol", {5, 1, {}, {TT_POL}}}};
  bool trunc = false;
  std::vector<const char *> a;
  for (int i = 1; i < argc; i++)
    if (!strcmp(argv[i], "--truncations")) trunc = true; else a.push_back(argv[i]);
  const Expect *kx = nullptr;
  for (const auto &k : kinds)
    if (a.size() >= 3 && !strcmp(a[2], k.name)) kx = &k.x;
  const bool image = a.size() >= 2 && !strcmp(a[1], "image");
  if (!kx || (!image && strcmp(a[1], "delta")) || a.size() != 3u + kx->nt) {
    fprintf(stderr, "usage: %s FILE image|delta nat|bridge|lb|fw|pol CAP [CAP2] [--truncations]\n",
            argv[0]);
    return 2;
  }
  Expect x = *kx;
  for (int k = 0; k < x.nt; k++) x.cap[k] = (uint32_t)strtoul(a[3 + k], nullptr, 0);
  FILE *fp = fopen(a[0], "rb");
  if (!fp) return perror(a[0]), 2;
  std::string all;
  char chunk[4096];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, fp)) > 0;) all.append(chunk, n);
  fclose(fp);
  const Format &f = image ? kImage : kDelta;
  char msg[256];
  for (size_t n = trunc ? 0 : all.size(); n <= all.size(); n++) {
    uint8_t *buf = (uint8_t *)malloc(n ? n : 1);
    memcpy(buf, all.data(), n);
    const int rc = check(f, x, buf, n, msg, sizeof msg);
    printf("%d %s\n", rc, msg);
    free(buf);
  }
  return 0;
}
