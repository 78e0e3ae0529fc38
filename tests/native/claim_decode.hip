/*
 * claim_decode.hip — the work-item decode of the kernels' claims (csrc/lane.h decode_item, decode_block,
 * take_from_block) on the host, for tests/test_claim_decode.py.  Built host-only.
 *
 * claim_decode_check fills KParams and the tile table the way hrt_render_tiles_device does (sample-chunk
 * schedule of a sphere scene, 8x8-block padding, the stride rule with HRT_TILE_STRIDE unset) and walks EVERY
 * work item w of the launch: the block decode of w's 64-aligned block plus take_from_block must give what the
 * per-item decode gives, every valid slot must lie inside the launch's output, every valid pixel inside its
 * tile, and each (pixel, chunk) must appear exactly once.  A wrong slot on the device is an out-of-bounds
 * store, so this is what stands between the decode and a GPU run.
 */
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "lane.h"

using namespace hrt;
using namespace hrt::lane;

extern "C" {

/* what the launch looked like, for the test's own assertions on the path it covered */
struct ClaimDecodeInfo {
  uint32_t total_work, pad_px, tile_stride, n_head, n_tail, chunk, chunk_first, n_out;
  uint32_t padding_items; /* items that are no pixel */
  uint32_t past_blocks;   /* 64-item blocks wholly past their tile (stride padding: BlockDesc.rh == 0) */
  uint32_t fail_w;        /* the first item that failed */
  uint32_t fail_what;     /* 0 none, 1 valid differs, 2 pxy, 3 slot, 4 samples, 5 slot out of range, 6 pixel outside its
                             tile, 7 (pixel, chunk) twice, 8 (pixel, chunk) missing, 9 a multiple-of-64 rule broken */
};

int claim_decode_check(const hrt_tile* tiles, uint32_t n_tiles, uint32_t W, uint32_t H, uint32_t spp, ClaimDecodeInfo* out) {
  ClaimDecodeInfo I;
  memset(&I, 0, sizeof(I));
  auto fail = [&](uint32_t w, uint32_t what) {
    I.fail_w = w;
    I.fail_what = what;
    *out = I;
    return 1;
  };
  /* hrt_render_tiles_device: chunk_schedule with the scene options' defaults */
  uint32_t chunk = 0, n_head = 0, first = 0, n_tail = 0;
  frame_chunks(spp, CHUNK_SPHERE, W, H, 0u, 0u, 32u, chunk, n_head, first, n_tail);
  const uint32_t n_chunks = n_head + n_tail;
  std::vector<G::TileDev> td(n_tiles);
  uint64_t pad = 0, outp = 0;
  for (uint32_t i = 0; i < n_tiles; i++) {
    const hrt_tile& t = tiles[i];
    if (t.w == 0 || t.h == 0 || (uint64_t)t.x + t.w > W || (uint64_t)t.y + t.h > H) return -1;
    const uint32_t bw = (t.w + 7) / 8, bh = (t.h + 7) / 8;
    td[i] = G::TileDev{t.x, t.y, t.w, t.h, bw, (uint32_t)pad, (uint32_t)outp, 0};
    pad += (uint64_t)bw * bh * 64;
    outp += (uint64_t)t.w * t.h;
  }
  uint32_t stride = 0;
  if (n_tiles > 1) {
    uint64_t mx = 0;
    for (uint32_t i = 0; i < n_tiles; i++) mx = std::max<uint64_t>(mx, (uint64_t)((td[i].w + 7) / 8) * ((td[i].h + 7) / 8) * 64);
    if (mx * n_tiles <= pad + pad / 8 && mx * n_tiles * n_chunks < 0xF0000000ull) {
      stride = (uint32_t)mx;
      for (uint32_t i = 0; i < n_tiles; i++) td[i].pad_start = i * stride;
      pad = mx * n_tiles;
    }
  }
  if (pad * n_chunks >= 0xF0000000ull) return -1;
  KParams P;
  memset(&P, 0, sizeof(P));
  P.W = W;
  P.H = H;
  P.spp = spp;
  P.tiles = td.data();
  P.n_tiles = n_tiles;
  P.total_work = (uint32_t)(pad * n_chunks);
  P.pad_px = (uint32_t)pad;
  P.head_items = (uint32_t)(pad * n_head);
  P.tile_stride = stride;
  P.chunk = chunk;
  P.n_chunks = n_chunks;
  P.chunk_head = n_head;
  P.chunk_first = first;
  P.n_out = (uint32_t)outp;
  I.total_work = P.total_work;
  I.pad_px = P.pad_px;
  I.tile_stride = stride;
  I.n_head = n_head;
  I.n_tail = n_tail;
  I.chunk = chunk;
  I.chunk_first = first;
  I.n_out = P.n_out;
  /* what makes a 64-aligned block uniform */
  if (P.total_work % 64u || P.pad_px % 64u || P.head_items % 64u || stride % 64u) return fail(0, 9);
  for (uint32_t i = 0; i < n_tiles; i++)
    if (td[i].pad_start % 64u) return fail(0, 9);

  /* the chunks' sample ranges: s0 identifies the chunk */
  std::vector<uint32_t> c0(n_chunks), c1(n_chunks);
  for (uint32_t k = 0; k < n_chunks; k++) chunk_range(P, k, c0[k], c1[k]);
  const uint64_t n_slots = (uint64_t)n_chunks * P.n_out;
  std::vector<uint8_t> seen(n_slots, 0);
  BlockDesc d;
  memset(&d, 0, sizeof(d));
  for (uint32_t w = 0; w < P.total_work; w++) {
    if ((w & 63u) == 0u) {
      decode_block(P, w, P.chunk_head, P.pad_px, P.tile_stride, d);
      if (d.rh == 0u) I.past_blocks++;
    }
    bool v_item = false;
    uint32_t pxy_i = 0, slot_i = 0, s0_i = 0, s1_i = 0;
    decode_item(P, w, P.chunk_head, P.pad_px, P.tile_stride, v_item, pxy_i, slot_i, s0_i, s1_i);
    uint32_t pxy_b = 0, slot_b = 0, s0_b = 0, s1_b = 0;
    const bool v_blk = take_from_block(d, w, pxy_b, slot_b, s0_b, s1_b);
    if (v_item != v_blk) return fail(w, 1);
    if (!v_item) {
      I.padding_items++;
      continue;
    }
    if (pxy_i != pxy_b) return fail(w, 2);
    if (slot_i != slot_b) return fail(w, 3);
    if (s0_i != s0_b || s1_i != s1_b) return fail(w, 4);
    if (slot_b >= n_slots) return fail(w, 5);
    /* the pixel's tile (tiles of one call are disjoint), and its own (pixel, chunk) slot worked out from the tile list */
    const uint32_t x = pxy_b & 0xFFFFu, y = pxy_b >> 16;
    uint32_t ti = n_tiles;
    uint64_t off = 0;
    for (uint32_t i = 0; i < n_tiles; i++) {
      const hrt_tile& t = tiles[i];
      if (x >= t.x && x < t.x + t.w && y >= t.y && y < t.y + t.h) {
        ti = i;
        break;
      }
      off += (uint64_t)t.w * t.h;
    }
    if (ti == n_tiles) return fail(w, 6);
    uint32_t k = n_chunks;
    for (uint32_t j = 0; j < n_chunks; j++)
      if (c0[j] == s0_b && c1[j] == s1_b) k = j;
    if (k == n_chunks) return fail(w, 4);
    const uint64_t want = (uint64_t)k * P.n_out + off + (uint64_t)(y - tiles[ti].y) * tiles[ti].w + (x - tiles[ti].x);
    if (want != slot_b) return fail(w, 3);
    if (seen[want]) return fail(w, 7);
    seen[want] = 1;
  }
  for (uint64_t s = 0; s < n_slots; s++)
    if (!seen[s]) return fail((uint32_t)s, 8);
  *out = I;
  return 0;
}

}  // extern "C"
