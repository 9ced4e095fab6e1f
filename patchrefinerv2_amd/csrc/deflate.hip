// zlib streams (RFC 1950 / 1951) of byte buffers that are already on the device (include/prv2.h "Device deflate"): the IDAT payload
// of the PNG files the output stage writes, so that only compressed bytes cross PCIe.  Frames convention of output.hip: rows
// [n, rows_fstride] with len valid bytes per frame; three launches per call, no host synchronisation, bit-deterministic.
//
//   deflate_seg_kernel   one workgroup per segment of kSeg input bytes; no match crosses a segment boundary.
//     LZ77     the segment lives in LDS.  Positions are taken in order, kChunk = 256 at a time (one per lane).  A lane looks its
//              4-byte hash up in a table of most recent positions that holds EARLIER chunks only, and tries distances 1 to 4 as well; all
//              candidates are verified byte for byte (length 3..258).  After a barrier the chunk's positions go into the table with
//              an LDS atomicMax (an ordered integer atomic: the result does not depend on which lane arrives first).  The greedy,
//              non-overlapping parse of the chunk is the set of positions reachable from the carried-in cursor through
//              p -> p + max(1, match length): marked with pointer doubling (8 rounds for 256 positions).
//     Huffman  every kSub = 4096 positions form one deflate block with dynamic codes.  Code lengths: the multiset of Shannon lengths
//              ceil(log2(total / f)) (Kraft sum <= 1, at most 13 bits for <= 4097 tokens), clamped to the alphabet's limit, moved to a
//              Kraft sum of exactly 1 on the length counts, and handed out in order of frequency; canonical codes; the run-length
//              coded header; bit positions from a prefix sum over the token lengths; LSB-first packing with LDS atomicOr.
//     Stored   a segment whose blocks do not beat 5 + seglen bytes is written as one stored block instead.
//     Every segment but the last ends with an empty stored block (zlib's sync flush), so segments are whole bytes.
//   deflate_scan_kernel  per frame: exclusive scan of the segment sizes, Adler-32 from the per-segment (sum, weighted sum) pairs,
//                        the 2-byte header, the trailer and the stream's byte count.
//   deflate_copy_kernel  compaction of the per-segment slots into one contiguous stream.
//
// Static LDS of deflate_seg_kernel: 64 528 bytes (two workgroups per CU).
#include <limits.h>

#include "common.h"

namespace prv2 {
namespace {

constexpr int kSeg = 32768;        // input bytes per segment == the deflate window: every distance inside a segment is legal
constexpr int kChunk = 256;        // positions per parse step, one per lane
constexpr int kSub = 4096;         // positions per deflate block
constexpr int kHashBits = 12;
constexpr int kSlot = kSeg + 16;   // bytes of a segment's slot in the workspace (5 + kSeg rounded up to 16)
constexpr int kOutWords = (kSub + 258 + 64) / 4 + 4;  // LDS staging of one block's bits
constexpr int kOutBits = (kOutWords - 3) * 32 - 64;   // the largest block that is staged
constexpr int kMaxEnt = 320;       // code-length symbols of a header: at most 286 + 30
constexpr uint32_t kAdler = 65521;

struct SegMeta {
  uint32_t size, a, b, off;  // bytes of the segment's stream; sum of its input bytes, position-weighted sum (both mod 65521); offset in the frame's stream
};

// block-uniform scalars kept in LDS
enum { S_NEXT, S_TOT, S_NUSED, S_BITS, S_A, S_B, S_HLIT, S_HDIST, S_NENT, S_HCLEN, S_COUNT };

struct Lds {
  uint32_t in[kSeg / 4 + 4];          // the segment, zero behind seglen
  uint32_t htab[1 << kHashBits];      // position + 1 of the most recent occurrence of a hash; 0: none
  uint32_t mtok[kSub / 3 + 2];        // match of the token at block position q, at q / 3 (matches start >= 3 apart): len - 3 | dist << 8
  uint32_t vis[kSub / 32], ism[kSub / 32];  // per block position: a token starts here / it is a match
  uint32_t outw[kOutWords];
  uint32_t hl[288], hd[32], hc[20];   // histograms: literal/length, distance, code-length alphabet
  uint16_t lcode[288], dcode[32], ccode[20];  // bit-reversed canonical codes
  uint8_t ll[288], dl[32], cl[20];    // code lengths
  uint32_t blc[16];                   // symbols per code length
  union {
    struct {
      uint16_t ja[kChunk], jb[kChunk];
      uint8_t vf[kChunk];
    } c;                              // parse: jump tables of the pointer doubling, visited flags
    struct {
      uint32_t scan[256];
      uint16_t ent[kMaxEnt];          // header: code-length symbol | extra bits << 5
    } e;                              // emission
  } u;
  uint32_t s[16];
};

__device__ __forceinline__ uint32_t ld32(const uint32_t* w, int p) {  // 4 bytes at any byte offset of a word array
  const uint64_t v = (uint64_t)w[p >> 2] | ((uint64_t)w[(p >> 2) + 1] << 32);
  return (uint32_t)(v >> (8 * (p & 3)));
}

// equal bytes at a.. and b.. (a < b), at most maxl; bytes behind the segment are never counted (maxl <= seglen - b)
__device__ __forceinline__ int match_len(const uint32_t* w, int a, int b, int maxl) {
  int i = 0;
  while (i < maxl) {
    const uint32_t x = ld32(w, a + i) ^ ld32(w, b + i);
    if (x) {
      i += (__ffs((int)x) - 1) >> 3;
      break;
    }
    i += 4;
  }
  return i < maxl ? i : maxl;
}

__device__ __forceinline__ uint32_t hash4(uint32_t x) { return (x * 2654435761u) >> (32 - kHashBits); }

// RFC 1951 3.2.5: symbol, extra-bit count and extra-bit value of a length 3..258 / a distance 1..32768
__device__ __forceinline__ void len_code(int len, int& sym, int& eb, int& ev) {
  const int x = len - 3;
  if (len == 258) {
    sym = 285, eb = 0, ev = 0;
  } else if (x < 8) {
    sym = 257 + x, eb = 0, ev = 0;
  } else {
    const int hb = 31 - __clz(x);
    eb = hb - 2;
    sym = 257 + 4 * (hb - 1) + ((x >> eb) & 3);
    ev = x & ((1 << eb) - 1);
  }
}
__device__ __forceinline__ void dist_code(int dist, int& sym, int& eb, int& ev) {
  const int x = dist - 1;
  if (x < 4) {
    sym = x, eb = 0, ev = 0;
  } else {
    const int hb = 31 - __clz(x);
    eb = hb - 1;
    sym = 2 * hb + ((x >> eb) & 1);
    ev = x & ((1 << eb) - 1);
  }
}
__device__ __forceinline__ int len_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
__device__ __forceinline__ int dist_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
__device__ __forceinline__ int cl_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// n <= 48 bits of val at bit position pos of the staging buffer, LSB first (atomicOr: neighbours share boundary words)
__device__ __forceinline__ void put_bits(uint32_t* outw, uint32_t pos, uint64_t val, int n) {
  if (n <= 0) return;
  const uint32_t w = pos >> 5, sh = pos & 31;
  const uint64_t lo = val << sh;
  const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = sh ? (uint32_t)(val >> (64 - sh)) : 0u;
  if (w0 && w < (uint32_t)kOutWords) atomicOr(&outw[w], w0);
  if (w1 && w + 1 < (uint32_t)kOutWords) atomicOr(&outw[w + 1], w1);
  if (w2 && w + 2 < (uint32_t)kOutWords) atomicOr(&outw[w + 2], w2);
}

// exclusive prefix sum over the workgroup's 256 lanes; *total = the sum
__device__ uint32_t block_scan(uint32_t v, uint32_t* sc, uint32_t* total) {
  const int tid = threadIdx.x;
  sc[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t t = tid >= off ? sc[tid - off] : 0u;
    __syncthreads();
    sc[tid] += t;
    __syncthreads();
  }
  const uint32_t incl = sc[tid];
  *total = sc[255];
  __syncthreads();
  return incl - v;
}

// Code lengths (<= maxbits) and bit-reversed canonical codes of an alphabet of n <= 288 symbols from its histogram.  No used symbol:
// all lengths 0; one: length 1 (an incomplete code, which inflate accepts for the literal/length and distance alphabets only, so
// ``complete`` gives the code-length alphabet a second symbol).  Otherwise the code is complete: Kraft sum exactly 1.
__device__ void build_code(Lds& L, uint32_t* freq, int n, int maxbits, uint8_t* lens, uint16_t* codes, bool complete) {
  const int tid = threadIdx.x;
  if (tid < 16) L.blc[tid] = 0;
  if (tid == 0) L.s[S_TOT] = 0, L.s[S_NUSED] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    lens[i] = 0;
    if (freq[i]) atomicAdd(&L.s[S_TOT], freq[i]), atomicAdd(&L.s[S_NUSED], 1u);
  }
  __syncthreads();
  const uint32_t nused0 = L.s[S_NUSED];
  __syncthreads();
  if (complete && nused0 == 1 && tid == 0) {
    freq[freq[0] ? 1 : 0] = 1;
    L.s[S_TOT] += 1;
    L.s[S_NUSED] = 2;
  }
  __syncthreads();
  const uint32_t total = L.s[S_TOT], nused = L.s[S_NUSED];
  if (nused == 0) return;
  if (nused == 1) {
    for (int i = tid; i < n; i += 256)
      if (freq[i]) lens[i] = 1, codes[i] = 0;
    __syncthreads();
    return;
  }
  // rank by (frequency descending, symbol ascending) and the Shannon length of every used symbol
  int rank[2] = {0, 0};
  for (int k = 0, i = tid; i < n; i += 256, ++k) {
    const uint32_t fi = freq[i];
    if (!fi) continue;
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t fj = freq[j];
      r += (fj > fi || (fj == fi && j < i)) ? 1 : 0;
    }
    rank[k] = r;
    int l = 1;
    while (l < maxbits && ((uint64_t)fi << l) < (uint64_t)total) ++l;
    atomicAdd(&L.blc[l], 1u);
  }
  __syncthreads();
  if (tid == 0) {  // the length counts to a Kraft sum of exactly 1 (units of 2^-maxbits)
    int K = 1 << maxbits;
    for (int l = 1; l <= maxbits; ++l) K -= (int)L.blc[l] << (maxbits - l);
    while (K < 0) {  // over-subscribed (only after the clamp to maxbits): lengthen the longest code below the limit
      int l = maxbits - 1;
      while (l > 0 && L.blc[l] == 0) --l;
      if (l == 0) break;
      L.blc[l] -= 1, L.blc[l + 1] += 1;
      K += 1 << (maxbits - l - 1);
    }
    while (K > 0) {  // incomplete: shorten the shortest code the slack pays for (the longest codes always qualify)
      int l = 2;
      while (l <= maxbits && (L.blc[l] == 0 || (1 << (maxbits - l)) > K)) ++l;
      if (l > maxbits) break;
      L.blc[l] -= 1, L.blc[l - 1] += 1;
      K -= 1 << (maxbits - l);
    }
  }
  __syncthreads();
  for (int k = 0, i = tid; i < n; i += 256, ++k) {
    if (!freq[i]) continue;
    uint32_t cum = 0;
    int l = 1;
    for (; l < maxbits; ++l) {
      cum += L.blc[l];
      if ((uint32_t)rank[k] < cum) break;
    }
    lens[i] = (uint8_t)l;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int l = lens[i];
    if (!l) continue;
    uint32_t code = 0;
    for (int b = 1; b <= l; ++b) code = (code + (b > 1 ? L.blc[b - 1] : 0u)) << 1;
    for (int j = 0; j < i; ++j) code += lens[j] == l ? 1u : 0u;
    codes[i] = (uint16_t)(__brev(code) >> (32 - l));
  }
  __syncthreads();
}

// bits of the token that starts at block position q (its segment position p): literal, or length + distance
__device__ __forceinline__ int token_bits(const Lds& L, int q, int p, uint64_t& val) {
  if (!((L.vis[q >> 5] >> (q & 31)) & 1u)) return 0;
  if (!((L.ism[q >> 5] >> (q & 31)) & 1u)) {
    const int b = (int)(ld32(L.in, p) & 0xFFu);
    val = L.lcode[b];
    return L.ll[b];
  }
  const uint32_t m = L.mtok[q / 3];
  int ls, le, lv, ds, de, dv;
  len_code((int)(m & 0xFFu) + 3, ls, le, lv);
  dist_code((int)(m >> 8), ds, de, dv);
  int n = L.ll[ls];
  uint64_t v = L.lcode[ls];
  v |= (uint64_t)lv << n;
  n += le;
  v |= (uint64_t)L.dcode[ds] << n;
  n += L.dl[ds];
  v |= (uint64_t)dv << n;
  n += de;
  val = v;
  return n;
}

__global__ void __launch_bounds__(256) deflate_seg_kernel(const uint8_t* __restrict__ rows, int64_t len, int64_t rows_fstride, int nseg,
                                                          uint8_t* __restrict__ slots, SegMeta* __restrict__ meta) {
  __shared__ Lds L;
  const int tid = threadIdx.x, seg = blockIdx.x, f = blockIdx.y;
  const int64_t s0 = (int64_t)seg * kSeg;
  const int64_t left = len - s0;
  const int seglen = left <= 0 ? 0 : left < kSeg ? (int)left : kSeg;
  const bool last = seg == nseg - 1;
  const uint8_t* src = rows + (int64_t)f * rows_fstride + s0;
  uint32_t* slot = (uint32_t*)(slots + ((int64_t)f * nseg + seg) * kSlot);

  // the segment into LDS (16-byte loads stay inside the frame: rows_fstride is a multiple of 16 and >= len); Adler partial sums
  uint32_t a_sum = 0, b_sum = 0;
  for (int v = tid; v < kSeg / 16; v += 256) {
    const int i0 = v * 16;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (i0 < seglen) q = *(const uint4*)(src + i0);
    uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int nv = seglen - (i0 + 4 * k);  // valid bytes of this word
      if (nv < 4) w[k] = nv <= 0 ? 0u : w[k] & ((1u << (8 * nv)) - 1u);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t byte = (w[k] >> (8 * b)) & 0xFFu;
        a_sum += byte;
        b_sum += byte * (uint32_t)(seglen - (i0 + 4 * k + b));  // a zero byte behind seglen adds nothing
      }
      L.in[v * 4 + k] = w[k];
    }
  }
  if (tid < 4) L.in[kSeg / 4 + tid] = 0;
  for (int i = tid; i < (1 << kHashBits); i += 256) L.htab[i] = 0;
  for (int i = tid; i < kOutWords; i += 256) L.outw[i] = 0;
  if (tid < 16) L.s[tid] = 0;
  __syncthreads();
  atomicAdd(&L.s[S_A], a_sum);
  atomicAdd(&L.s[S_B], b_sum % kAdler);
  __syncthreads();

  bool giveup = seglen == 0;  // block-uniform from here on
  int nextp = 0;              // the parse cursor: first position no token covers yet
  uint32_t gbits = 0;         // bits of the segment's stream so far; L.outw[0] holds the bits of its last, partial word
  for (int b0 = 0; b0 < seglen && !giveup; b0 += kSub) {
    const int b1 = b0 + kSub < seglen ? b0 + kSub : seglen;
    for (int i = tid; i < 288; i += 256) L.hl[i] = 0;
    if (tid < 32) L.hd[tid] = 0;
    if (tid < 20) L.hc[tid] = 0;
    if (tid < kSub / 32) L.vis[tid] = 0, L.ism[tid] = 0;
    __syncthreads();

    // ---- LZ77 over the block's positions, a chunk at a time
    for (int c0 = b0; c0 < b1; c0 += kChunk) {
      const int p = c0 + tid;
      const bool valid = p < seglen;
      int mlen = 0, dist = 0;
      uint32_t h = 0;
      bool ins = false;
      if (valid) {
        const int maxl = seglen - p < 258 ? seglen - p : 258;
        if (maxl >= 4) {
          h = hash4(ld32(L.in, p));
          ins = true;
          const uint32_t cand = L.htab[h];  // earlier chunks only: this chunk is inserted behind the barrier
          if (cand) {
            const int c = (int)cand - 1;
            const int l = match_len(L.in, c, p, maxl);
            if (l >= 4 || (l == 3 && p - c <= 4096)) mlen = l, dist = p - c;
          }
        }
        if (maxl >= 3) {  // distances 4 .. 1: runs and repeated pixels, which the table of earlier chunks cannot see inside a chunk
          const uint32_t here = ld32(L.in, p) & 0xFFFFFFu;
          for (int d = 4; d >= 1; --d) {
            if (p < d || (ld32(L.in, p - d) & 0xFFFFFFu) != here) continue;
            const int l = match_len(L.in, p - d, p, maxl);
            if (l >= 3 && l >= mlen) mlen = l, dist = d;
          }
        }
      }
      const int tgt = p + (mlen >= 3 ? mlen : 1);
      const int start = nextp - c0;  // >= 0
      L.u.c.ja[tid] = (uint16_t)(tgt - c0 < kChunk ? tgt - c0 : kChunk);
      L.u.c.vf[tid] = tid == start ? 1 : 0;
      const int any = __syncthreads_or(mlen >= 3 ? 1 : 0);
      if (ins) atomicMax(&L.htab[h], (uint32_t)(p + 1));
      bool v;
      if (!any) {  // literals only: every position from the cursor on
        v = tid >= start;
      } else {     // positions reachable from the cursor: V <- V u J(V), J <- J o J
        uint16_t* cur = L.u.c.ja;
        uint16_t* nxt = L.u.c.jb;
        for (int r = 0; r < 8; ++r) {
          const bool vv = L.u.c.vf[tid] != 0;
          const int j = cur[tid];
          const int jj = j < kChunk ? cur[j] : kChunk;
          __syncthreads();
          if (vv && j < kChunk) L.u.c.vf[j] = 1;
          nxt[tid] = (uint16_t)jj;
          __syncthreads();
          uint16_t* t = cur;
          cur = nxt;
          nxt = t;
        }
        v = L.u.c.vf[tid] != 0;
      }
      if (v && tgt >= c0 + kChunk) L.s[S_NEXT] = (uint32_t)tgt;  // the one visited position whose token leaves the chunk
      if (v && valid) {
        const int q = p - b0;
        atomicOr(&L.vis[q >> 5], 1u << (q & 31));
        if (mlen >= 3) {
          atomicOr(&L.ism[q >> 5], 1u << (q & 31));
          L.mtok[q / 3] = (uint32_t)(mlen - 3) | ((uint32_t)dist << 8);
          int sym, eb, ev;
          len_code(mlen, sym, eb, ev);
          atomicAdd(&L.hl[sym], 1u);
          dist_code(dist, sym, eb, ev);
          atomicAdd(&L.hd[sym], 1u);
        } else {
          atomicAdd(&L.hl[ld32(L.in, p) & 0xFFu], 1u);
        }
      }
      __syncthreads();
      nextp = (int)L.s[S_NEXT];
    }
    if (tid == 0) L.hl[256] += 1;  // end of block
    __syncthreads();

    // ---- codes and the header
    build_code(L, L.hl, 286, 15, L.ll, L.lcode, false);
    build_code(L, L.hd, 30, 15, L.dl, L.dcode, false);
    if (tid == 0) {  // run-length coding of the hlit + hdist code lengths (RFC 1951 3.2.7)
      int hlit = 286, hdist = 30;
      while (hlit > 257 && L.ll[hlit - 1] == 0) --hlit;
      while (hdist > 1 && L.dl[hdist - 1] == 0) --hdist;
      const int N = hlit + hdist;
      int ne = 0, i = 0;
      while (i < N) {
        const int v = i < hlit ? L.ll[i] : L.dl[i - hlit];
        int run = 1;
        while (i + run < N && (i + run < hlit ? L.ll[i + run] : L.dl[i + run - hlit]) == v) ++run;
        i += run;
        if (v == 0) {
          while (run >= 11) {
            const int r = run < 138 ? run : 138;
            L.u.e.ent[ne++] = (uint16_t)(18 | ((r - 11) << 5)), L.hc[18] += 1;
            run -= r;
          }
          if (run >= 3) {
            L.u.e.ent[ne++] = (uint16_t)(17 | ((run - 3) << 5)), L.hc[17] += 1;
            run = 0;
          }
        } else {
          L.u.e.ent[ne++] = (uint16_t)v, L.hc[v] += 1;
          --run;
          while (run >= 3) {
            const int r = run < 6 ? run : 6;
            L.u.e.ent[ne++] = (uint16_t)(16 | ((r - 3) << 5)), L.hc[16] += 1;
            run -= r;
          }
        }
        for (; run > 0; --run) L.u.e.ent[ne++] = (uint16_t)v, L.hc[v] += 1;
      }
      L.s[S_HLIT] = hlit, L.s[S_HDIST] = hdist, L.s[S_NENT] = ne;
    }
    __syncthreads();
    build_code(L, L.hc, 19, 7, L.cl, L.ccode, true);
    const int kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    if (tid == 0) {
      int hclen = 19;
      while (hclen > 4 && L.cl[kOrder[hclen - 1]] == 0) --hclen;
      L.s[S_HCLEN] = hclen;
      L.s[S_BITS] = 17 + 3 * hclen;
    }
    __syncthreads();
    const int hlit = (int)L.s[S_HLIT], hdist = (int)L.s[S_HDIST], nent = (int)L.s[S_NENT], hclen = (int)L.s[S_HCLEN];
    {  // the block's size in bits
      uint32_t bits = 0;
      for (int i = tid; i < 286; i += 256) bits += L.hl[i] * (uint32_t)(L.ll[i] + len_extra(i));
      if (tid < 30) bits += L.hd[tid] * (uint32_t)(L.dl[tid] + dist_extra(tid));
      for (int i = tid; i < nent; i += 256) bits += (uint32_t)(L.cl[L.u.e.ent[i] & 31] + cl_extra(L.u.e.ent[i] & 31));
      if (bits) atomicAdd(&L.s[S_BITS], bits);
    }
    __syncthreads();
    const uint32_t dyn = L.s[S_BITS];
    // a block that does not fit the staging buffer, or a stream that cannot beat the stored form any more: store the segment
    if (dyn > (uint32_t)kOutBits || (gbits + dyn + 7) / 8 + 12 > (uint32_t)(5 + seglen)) {
      giveup = true;
      break;
    }

    // ---- emission into the staging buffer at bit position pos
    const uint32_t pos = gbits & 31;
    if (tid == 0) {
      const uint32_t bfinal = last && b1 == seglen ? 1u : 0u;
      put_bits(L.outw, pos, bfinal | (2u << 1) | ((uint32_t)(hlit - 257) << 3) | ((uint32_t)(hdist - 1) << 8) | ((uint32_t)(hclen - 4) << 13), 17);
      for (int k = 0; k < hclen; ++k) put_bits(L.outw, pos + 17 + 3 * k, L.cl[kOrder[k]], 3);
    }
    uint32_t cursor = pos + 17 + 3 * hclen, total;
    {  // header entries, two per lane
      uint32_t nb = 0;
      for (int k = 0; k < 2; ++k) {
        const int e = 2 * tid + k;
        if (e < nent) nb += (uint32_t)(L.cl[L.u.e.ent[e] & 31] + cl_extra(L.u.e.ent[e] & 31));
      }
      // (the scan scratch does not overlap the entries: both live in u.e)
      uint32_t at = cursor + block_scan(nb, L.u.e.scan, &total);
      for (int k = 0; k < 2; ++k) {
        const int e = 2 * tid + k;
        if (e >= nent) break;
        const int sym = L.u.e.ent[e] & 31, x = L.u.e.ent[e] >> 5, n = L.cl[sym];
        put_bits(L.outw, at, (uint64_t)L.ccode[sym] | ((uint64_t)x << n), n + cl_extra(sym));
        at += n + cl_extra(sym);
      }
      cursor += total;
    }
    {  // tokens, kSub / 256 consecutive positions per lane
      constexpr int per = kSub / 256;
      uint32_t nb = 0;
      uint64_t val = 0;
      for (int k = 0; k < per; ++k) {
        const int q = tid * per + k;
        if (b0 + q < b1) nb += (uint32_t)token_bits(L, q, b0 + q, val);
      }
      uint32_t at = cursor + block_scan(nb, L.u.e.scan, &total);
      for (int k = 0; k < per; ++k) {
        const int q = tid * per + k;
        if (b0 + q >= b1) break;
        const int n = token_bits(L, q, b0 + q, val);
        put_bits(L.outw, at, val, n);
        at += n;
      }
      cursor += total;
    }
    if (tid == 0) put_bits(L.outw, cursor, L.lcode[256], L.ll[256]);
    __syncthreads();

    // ---- whole words to the slot; the partial word stays
    const uint32_t cw = (pos + dyn) >> 5, gw0 = gbits >> 5;
    for (uint32_t i = tid; i < cw; i += 256)
      if (gw0 + i < (uint32_t)(kSlot / 4)) slot[gw0 + i] = L.outw[i];
    const uint32_t carry = cw < (uint32_t)kOutWords ? L.outw[cw] : 0u;
    __syncthreads();
    for (uint32_t i = tid; i <= cw + 2 && i < (uint32_t)kOutWords; i += 256) L.outw[i] = i == 0 ? carry : 0u;
    __syncthreads();
    gbits += dyn;
  }

  uint32_t size;
  if (!giveup) {
    // byte alignment: an empty stored block (000, pad, 00 00 FF FF) behind every segment but the last, zero bits behind the last
    const uint32_t pos = gbits & 31;
    uint32_t end = gbits;
    if (!last) {
      end = (gbits + 3 + 7) / 8 * 8;
      if (tid == 0) put_bits(L.outw, pos + (end - gbits), 0xFFFF0000u, 32);
      end += 32;
    } else {
      end = (gbits + 7) / 8 * 8;
    }
    __syncthreads();
    const uint32_t nw = (pos + (end - gbits) + 31) >> 5, gw0 = gbits >> 5;
    for (uint32_t i = tid; i < nw; i += 256)
      if (gw0 + i < (uint32_t)(kSlot / 4) && i < (uint32_t)kOutWords) slot[gw0 + i] = L.outw[i];
    size = end / 8;
    if (size >= (uint32_t)(5 + seglen)) giveup = true;
    __syncthreads();  // (the slot is rewritten below by other lanes than those that wrote it here)
  }
  if (giveup) {  // one stored block: BFINAL, LEN, ~LEN, the bytes (seglen <= 32768 < 65536)
    size = 5 + seglen;
    const uint32_t hdr = (last ? 1u : 0u) | ((uint32_t)seglen << 8) | ((~(uint32_t)seglen & 0xFFu) << 24);
    const int words = (5 + seglen + 3) / 4;
    for (int k = tid; k < words; k += 256) {
      uint32_t w;
      if (k == 0) w = hdr;
      else if (k == 1) w = ((~(uint32_t)seglen >> 8) & 0xFFu) | (ld32(L.in, 0) << 8);
      else w = ld32(L.in, 4 * k - 5);
      slot[k] = w;
    }
  }
  if (tid == 0) {
    SegMeta m;
    m.size = size, m.a = L.s[S_A] % kAdler, m.b = L.s[S_B] % kAdler, m.off = 0;
    meta[(int64_t)f * nseg + seg] = m;
  }
}

// one workgroup per frame: where every segment goes, the zlib header, the Adler-32 trailer and the byte count
__global__ void __launch_bounds__(256) deflate_scan_kernel(SegMeta* __restrict__ meta, int nseg, int64_t len, uint8_t* __restrict__ out,
                                                           int64_t out_fstride, int64_t* __restrict__ out_bytes) {
  __shared__ uint32_t p_size[256], p_a[256], p_b[256], p_n[256], p_off[256];
  const int tid = threadIdx.x, f = blockIdx.x;
  SegMeta* m = meta + (int64_t)f * nseg;
  const int per = (nseg + 255) / 256;
  const int lo = tid * per < nseg ? tid * per : nseg, hi = lo + per < nseg ? lo + per : nseg;
  uint32_t size = 0, a = 0, b = 0, n = 0;  // a, b, n mod 65521: the lane's segments as one piece (sum, weighted sum, length)
  for (int s = lo; s < hi; ++s) {
    const int64_t left = len - (int64_t)s * kSeg;
    const uint32_t sl = left <= 0 ? 0u : left < kSeg ? (uint32_t)left : (uint32_t)kSeg;
    b = (uint32_t)(((uint64_t)b + (uint64_t)(sl % kAdler) * a + m[s].b) % kAdler);
    a = (a + m[s].a) % kAdler;
    n = (n + sl) % kAdler;
    size += m[s].size;
  }
  p_size[tid] = size, p_a[tid] = a, p_b[tid] = b, p_n[tid] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t off = 2, s1 = 1, s2 = 0;
    for (int t = 0; t < 256; ++t) {
      p_off[t] = off;
      off += p_size[t];
      s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)p_n[t] * s1 + p_b[t]) % kAdler);
      s1 = (s1 + p_a[t]) % kAdler;
    }
    uint8_t* o = out + (int64_t)f * out_fstride;
    o[0] = 0x78, o[1] = 0x01;  // deflate, 32 KiB window, no dictionary, fastest level
    o[off] = (uint8_t)(s2 >> 8), o[off + 1] = (uint8_t)s2, o[off + 2] = (uint8_t)(s1 >> 8), o[off + 3] = (uint8_t)s1;
    out_bytes[f] = (int64_t)off + 4;
  }
  __syncthreads();
  uint32_t off = p_off[tid];
  for (int s = lo; s < hi; ++s) {
    m[s].off = off;
    off += m[s].size;
  }
}

__global__ void __launch_bounds__(256) deflate_copy_kernel(const uint8_t* __restrict__ slots, const SegMeta* __restrict__ meta, int nseg,
                                                           uint8_t* __restrict__ out, int64_t out_fstride) {
  const int tid = threadIdx.x, seg = blockIdx.x, f = blockIdx.y;
  const SegMeta m = meta[(int64_t)f * nseg + seg];
  const int size = (int)m.size;
  if (size > kSlot - 8 || (int64_t)m.off + size + 4 > out_fstride) return;  // (never: the bound holds by construction)
  const uint8_t* sb = slots + ((int64_t)f * nseg + seg) * kSlot;
  const uint32_t* sw = (const uint32_t*)sb;
  uint8_t* d = out + (int64_t)f * out_fstride + m.off;
  int head = (int)((4 - ((uintptr_t)d & 3)) & 3);
  if (head > size) head = size;
  if (tid < head) d[tid] = sb[tid];
  const int nw = (size - head) >> 2;
  for (int w = tid; w < nw; w += 256) {
    const int p = head + 4 * w;
    const uint32_t w0 = sw[p >> 2];
    const uint32_t v = (p & 3) ? (uint32_t)((((uint64_t)sw[(p >> 2) + 1] << 32) | w0) >> (8 * (p & 3))) : w0;
    *(uint32_t*)(d + p) = v;
  }
  const int done = head + 4 * nw;
  if (tid < size - done) d[done + tid] = sb[done + tid];
}

static int64_t seg_count(int64_t len) { return len <= 0 ? 1 : cdiv(len, kSeg); }
static int64_t bound_of(int64_t len) { return roundup(6 + len + 10 * seg_count(len), 16); }

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int32_t prv2_deflate_segment(void) { return kSeg; }

extern "C" int64_t prv2_deflate_bound(int64_t len) {
  if (len < 0 || len > (int64_t)INT_MAX) return -1;
  return bound_of(len);
}

extern "C" int64_t prv2_deflate_workspace_bytes(int32_t n, int64_t len) {
  if (n < 1 || n > 65535 || len < 0 || len > (int64_t)INT_MAX) return -1;
  return (int64_t)n * seg_count(len) * (kSlot + (int64_t)sizeof(SegMeta));
}

extern "C" int prv2_deflate_rows(const uint8_t* rows, int32_t n, int64_t len, int64_t rows_fstride, uint8_t* out, int64_t out_fstride,
                                 int64_t* out_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "deflate_rows";
  PRV2_REQUIRE(rows && out && out_bytes, "%s: null pointer", name);
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(len >= 0 && len <= (int64_t)INT_MAX, "%s: length %lld out of range [0, 2^31)", name, (long long)len);
  PRV2_REQUIRE((((uintptr_t)rows | (uintptr_t)out) & 15) == 0 && ((uintptr_t)out_bytes & 7) == 0,
               "%s: rows and out must be 16-byte aligned, out_bytes 8-byte aligned", name);
  PRV2_REQUIRE(rows_fstride % 16 == 0 && rows_fstride >= len, "%s: frame stride %lld of rows: a multiple of 16, at least the length %lld", name,
               (long long)rows_fstride, (long long)len);
  PRV2_REQUIRE(out_fstride % 16 == 0 && out_fstride >= bound_of(len), "%s: frame stride %lld of out: a multiple of 16, at least %lld (prv2_deflate_bound)",
               name, (long long)out_fstride, (long long)bound_of(len));
  PRV2_REQUIRE(workspace != nullptr, "%s: null workspace", name);
  PRV2_REQUIRE(workspace_bytes >= prv2_deflate_workspace_bytes(n, len), "%s: workspace of %lld bytes < %lld (prv2_deflate_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)prv2_deflate_workspace_bytes(n, len));
  PRV2_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  const int nseg = (int)seg_count(len);
  uint8_t* slots = (uint8_t*)workspace;
  SegMeta* meta = (SegMeta*)(slots + (int64_t)n * nseg * kSlot);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(deflate_seg_kernel, dim3(nseg, n), dim3(256), 0, s, rows, len, rows_fstride, nseg, slots, meta);
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(n), dim3(256), 0, s, meta, nseg, len, out, out_fstride, out_bytes);
  hipLaunchKernelGGL(deflate_copy_kernel, dim3(nseg, n), dim3(256), 0, s, (const uint8_t*)slots, (const SegMeta*)meta, nseg, out, out_fstride);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
