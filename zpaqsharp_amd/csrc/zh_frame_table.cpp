// zh_frame_table.cpp — zh_frame.h's host side: BlockFrame, the store layout and the frame table of a batch.  Plain C++,
// no HIP: it links into libzpaqhip.so and, on its own, into the stand-alone test of the table.
#include <string.h>

#include <algorithm>

#include "zh_frame.h"

std::vector<uint8_t> zh::selector_prefix(const uint8_t *pcomp, size_t pcomp_len) {
  if (!pcomp_len) return {0};
  std::vector<uint8_t> sel{1, (uint8_t)(pcomp_len & 255), (uint8_t)(pcomp_len >> 8)};
  sel.insert(sel.end(), pcomp, pcomp + pcomp_len);
  return sel;
}

zh::BlockFrame::BlockFrame(bool tag, uint8_t level, const uint8_t *hdr, size_t hdr_len, const char *filename, uint64_t plain_len,
                           const uint32_t *digest, bool first, bool last) : tail(4, '\0') {
  static constexpr uint8_t kTag[13] = {0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3};   // Compressor.cs:27-43
  if (first) {
    if (tag) head.append((const char *)kTag, 13);
    head.append("zPQ", 3);
    head.push_back((char)level);
    head.push_back(1);
    head.append((const char *)hdr, hdr_len);
  }
  head.push_back(1);
  if (filename) head.append(filename);
  head.push_back(0);
  head.append(std::to_string(plain_len));
  head.push_back(0);
  head.push_back(0);
  if (digest) {
    tail.push_back((char)253);
    for (int w = 0; w < 5; ++w)
      for (int s = 24; s >= 0; s -= 8) tail.push_back((char)(digest[w] >> s));
  } else tail.push_back((char)254);
  if (last) tail.push_back((char)255);
}

uint64_t zh::store_body_len(uint64_t decoded) { return decoded + 4 * ((decoded + 65535) / 65536); }

void zh::write_store_body(uint8_t *w, const std::vector<uint8_t> &sel, const uint8_t *pre, uint64_t pre_len) {
  const uint64_t ns = sel.size(), dec = ns + pre_len;
  for (uint64_t c = 0; c < dec; c += 65536) {
    const uint64_t e = std::min<uint64_t>(c + 65536, dec), cl = e - c, p = std::max(c, ns);
    *w++ = (uint8_t)(cl >> 24); *w++ = (uint8_t)(cl >> 16); *w++ = (uint8_t)(cl >> 8); *w++ = (uint8_t)cl;
    if (c < ns) memcpy(w, sel.data() + c, std::min(ns, e) - c);
    if (p < e) memcpy(w + (p - c), pre + (p - ns), e - p);
    w += cl;
  }
}

uint64_t zh::build_frame_table(bool tag, uint8_t level, const uint8_t *hdr, size_t hdr_len, const std::vector<TableBlock> &items,
                               const std::vector<uint8_t> *sel, uint64_t pos, uint64_t out_cap, FrameTable &T, uint64_t *block_pos) {
  T = FrameTable();
  if (sel) {
    for (const TableBlock &it : items)
      if (it.seg.size() != 1) return kFrameRefused;
    T.blob = *sel;
    T.sel_len = sel->size();
  }
  for (size_t j = 0; j < items.size(); ++j) {
    const TableBlock &it = items[j];
    const size_t ns = it.seg.size(), e0 = T.entry.size(), blob0 = T.blob.size();
    uint64_t need = 0, from = 0;
    uint32_t pieces = T.pieces;
    for (size_t s = 0; s < ns; ++s) {
      const TableSeg &sg = it.seg[s];
      const BlockFrame f(tag, level, hdr, hdr_len, sg.filename, sg.plain_len, sg.digest, s == 0, s + 1 == ns);
      ZhFrameEntry e;
      memset(&e, 0, sizeof e);
      e.dst_off = pos + need;
      e.src = it.src;
      e.src_off = it.src_off + from;
      e.body_len = sg.end - from;
      e.store = sel ? 1 : 0;
      e.head_off = T.blob.size();
      e.head_len = (uint32_t)f.head.size();
      T.blob.insert(T.blob.end(), f.head.begin(), f.head.end());
      e.tail_off = T.blob.size();
      e.tail_len = (uint32_t)f.tail.size();
      T.blob.insert(T.blob.end(), f.tail.begin(), f.tail.end());
      T.entry.push_back(e);
      T.item.push_back(j);
      const uint64_t decoded = T.sel_len + e.body_len;
      need += f.head.size() + (sel ? store_body_len(decoded) : e.body_len) + f.tail.size();
      pieces = (uint32_t)std::max<uint64_t>(pieces, (decoded + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE);
      from = sg.end;
    }
    if (block_pos) block_pos[j] = pos;
    if (need <= out_cap && pos <= out_cap - need) T.pieces = pieces;
    else {                                // the whole block or nothing of it
      T.entry.resize(e0);
      T.item.resize(e0);
      T.blob.resize(blob0);
    }
    pos += need;
  }
  return pos;
}

uint64_t zh::build_gather_table(const std::vector<GatherItem> &items, uint64_t out_cap, FrameTable &T, uint64_t *block_pos) {
  T = FrameTable();
  uint64_t pos = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    const GatherItem &it = items[i];
    if (block_pos) block_pos[i] = pos;
    if (it.len <= out_cap && pos <= out_cap - it.len) {
      ZhFrameEntry e;
      memset(&e, 0, sizeof e);
      e.dst_off = pos;
      e.src = ZH_FRAME_SRC_FIRST;
      e.src_off = it.src_off;
      e.body_len = it.len;
      T.entry.push_back(e);
      T.item.push_back(i);
      T.pieces = (uint32_t)std::max<uint64_t>(T.pieces, (it.len + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE);
    }
    pos += it.len;
  }
  return pos;
}
