// The framing scan of device-resident streams (zh_scan_walk.h) on the host: the two lists from a plain loop, then the walk the
// GPU runs (a parse per tag hit, the chain, the segment fill), compared field by field with zh_framing.cpp's scan_stream.
// Built stand-alone with -fsanitize=address,undefined by tests/test_scan_walk.py; reads the cases from the file it is given
// ([u32 name length][name][u64 length][bytes] ...) and prints one line per case.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "zh_host.h"
#include "zh_scan_walk.h"

static int compare(const std::string &name, const std::vector<uint8_t> &in) {
  const uint8_t *p = in.data();
  const uint64_t n = in.size();
  // ---- the lists: every q whose 16-byte window has the hashes; every maximal run of four or more zero bytes
  std::vector<uint64_t> tag, rs, re;
  for (uint64_t q = 16; q <= n; ++q)
    if (zh_scan_tag_at(p, q)) tag.push_back(q);
  for (uint64_t i = 0; i < n;) {
    uint64_t j = i;
    while (j < n && p[j] == 0) ++j;
    if (j - i >= 4) { rs.push_back(i); re.push_back(j); }
    i = j > i ? j : i + 1;
  }
  const ZhScanLists L{tag.data(), rs.data(), re.data(), tag.size(), rs.size()};
  // ---- the walk
  std::vector<ZhScanRec> recs(tag.size());
  for (size_t i = 0; i < tag.size(); ++i) zh_scan_parse_block(p, n, L, tag[i], recs[i], nullptr, 0, 0);
  ZhScanResult R;
  std::vector<zpaqhip_block> blocks(tag.size() + 1);
  zh_scan_chain(p, n, L, recs.data(), blocks.data(), blocks.size(), R);
  if (R.n_blocks > blocks.size()) {
    blocks.resize(R.n_blocks);
    zh_scan_chain(p, n, L, recs.data(), blocks.data(), blocks.size(), R);
  }
  blocks.resize(R.n_blocks);
  std::vector<zpaqhip_segment> segs(R.n_segs);
  for (size_t b = 0; b < blocks.size(); ++b) zh_scan_fill_segments(p, n, L, blocks[b], (uint32_t)b, segs.data(), segs.size());
  // ---- the host scan
  zh::ScanOut so;
  zpaqhip_err e{};
  const int rc = zh::scan_stream(p, n, so, &e);
  std::string why;
  char buf[200];
#define CHECK(a, b, what) do { if ((a) != (b)) { snprintf(buf, sizeof buf, " %s %lld != %lld", what, (long long)(a), (long long)(b)); why += buf; } } while (0)
  CHECK(R.status, rc, "rc");
  CHECK(R.n_blocks, so.blocks.size(), "n_blocks");
  CHECK(R.n_segs, so.segs.size(), "n_segs");
  if (rc) {
    CHECK(R.err_block, e.block, "err.block");
    CHECK(R.err_seg, e.segment, "err.segment");
    if (strcmp(zh_scan_message(R.msg), e.msg) != 0) why += std::string(" msg '") + zh_scan_message(R.msg) + "' != '" + e.msg + "'";
    CHECK(R.hit_eof != 0, so.hit_eof, "hit_eof");
  }
  for (size_t b = 0; b < blocks.size() && b < so.blocks.size(); ++b) {
    const zpaqhip_block &x = blocks[b], &y = so.blocks[b];
    CHECK(x.tag_off, y.tag_off, "tag_off"); CHECK(x.hdr_off, y.hdr_off, "hdr_off"); CHECK(x.hdr_len, y.hdr_len, "hdr_len");
    CHECK(x.level, y.level, "level"); CHECK(x.n_comp, y.n_comp, "n_comp"); CHECK(x.hh, y.hh, "hh"); CHECK(x.hm, y.hm, "hm");
    CHECK(x.ph, y.ph, "ph"); CHECK(x.pm, y.pm, "pm"); CHECK(x.reserved, y.reserved, "reserved");
    CHECK(x.first_seg, y.first_seg, "first_seg"); CHECK(x.n_seg, y.n_seg, "n_seg"); CHECK(x.end_off, y.end_off, "end_off");
    CHECK(x.usize_hint, y.usize_hint, "usize_hint");
    if (x.model_mem != y.model_mem) why += " model_mem";
  }
  for (size_t s = 0; s < segs.size() && s < so.segs.size(); ++s) {
    const zpaqhip_segment &x = segs[s], &y = so.segs[s];
    CHECK(x.block, y.block, "seg.block"); CHECK(x.flags, y.flags, "flags"); CHECK(x.name_off, y.name_off, "name_off");
    CHECK(x.name_len, y.name_len, "name_len"); CHECK(x.comment_len, y.comment_len, "comment_len");
    CHECK(x.comment_off, y.comment_off, "comment_off"); CHECK(x.data_off, y.data_off, "data_off");
    CHECK(x.data_len, y.data_len, "data_len"); CHECK(x.usize_hint, y.usize_hint, "seg.usize_hint");
    CHECK(x.reserved, y.reserved, "seg.reserved");
    if (memcmp(x.sha1, y.sha1, 20) != 0) why += " sha1";
  }
  printf("%s %s rc=%d blocks=%zu segs=%zu tags=%zu runs=%zu%s\n", why.empty() ? "ok" : "FAIL", name.c_str(), rc, so.blocks.size(),
         so.segs.size(), tag.size(), rs.size(), why.c_str());
  return why.empty() ? 0 : 1;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int bad = 0, cases = 0;
  for (;;) {
    uint32_t nl = 0;
    uint64_t len = 0;
    if (fread(&nl, 4, 1, f) != 1) break;
    std::string name(nl, ' ');
    if (nl && fread(&name[0], 1, nl, f) != nl) return 2;
    if (fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> in((size_t)len);
    if (len && fread(in.data(), 1, (size_t)len, f) != len) return 2;
    bad += compare(name, in);
    ++cases;
  }
  fclose(f);
  printf("%d cases, %d failed\n", cases, bad);
  return bad ? 1 : 0;
}
