// Linking the instances of consecutive frames (gfx950): a sequence of int32 label
// maps (a time lapse, or the slices of a z-stack) becomes the same maps with one id
// per track, a lineage table and a status row.  No reference counterpart;
// tests/track_ref.py holds the rule in numpy on top of tests/match_ref.py.
//
// The rule works on the original ids of every frame, so the T - 1 frame pairs are
// independent.  Instance b of frame t >= 1 with area A_b has the partner a of highest
// IoU in frame t - 1 (match.hip: ties to the smaller id), intersection I, area A_a.
//   b continues the track of a   iff a exists, the best partner of a in frame t is b
//                                and I den > num (A_a + A_b - I)  (IoU > num / den);
//   otherwise b starts a track,  with parent = the track of a iff a exists and 2 I > A_b.
// Every instance of frame 0 starts a track without a parent.  Tracks are numbered from
// 1 in the order (first frame, original id).
//
// All passes are ordinary launches on the caller's stream, nothing is read back:
//
//   (1) launch_match_instances  per sequence, gt = frames 0..T-2, pred = frames 1..T-1
//                           of the same buffer (N = T - 1, no copies); the gt and pred
//                           tables and the status rows land in the workspace.  T == 1
//                           has no pair: frame 0 is matched against itself, which gives
//                           its areas (gt table, column 0) and its out_of_range count.
//   (2) link_resolve_kernel one block per sequence.  It zeroes the sequence's table,
//                           then walks t = 0..T-1; within a frame the ids 0..M go in
//                           chunks of kLinkBlock = 1024.  A thread decides continue / new /
//                           parent for its id from the table rows of pair t - 1 and
//                           lut[t-1]; the new tracks of a chunk are numbered by a ballot
//                           scan over the block, carried across chunks and frames, so
//                           the numbers ascend with the id.  It writes lut[t][id] (0 for
//                           id 0 and absent ids) and its track's table row.  The links
//                           are a matching: a track is continued by at most one id of a
//                           frame, so no two threads of a frame touch one row, and the
//                           frames are separated by block barriers (lut[t-1] and the
//                           rows were written by other threads of the same block).
//                           Every barrier is in block-uniform control flow: the loop
//                           bounds depend on T and M only.  Rows above max_tracks are
//                           not written.  The status row is written at the end.
//                           Latency-bound: T ceil((M + 1) / kLinkBlock) rounds of one
//                           block; small next to (1) and (3) and not tuned.
//   (3) link_relabel_kernel the bandwidth pass: tracks[p] = lut[t][labels[p]], 0 for a
//                           value outside 0..M.  A block takes kRelabelVecs 16-byte
//                           groups of one frame; the pixels before the first 16-byte
//                           boundary of the frame and after the last whole group go one
//                           by one (block 0).  The frame's LUT row is staged in LDS when
//                           max_instances <= kLinkLdsIds, else read through L2.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

constexpr int NT = kLinkBlock;       // threads of a resolve block = ids per chunk
constexpr int RT = 256;              // threads of a relabel block
constexpr int kRelabelVecs = 4096;   // 16-byte groups per relabel block: 64 KiB read, 64 KiB written
static_assert(NT % 64 == 0 && NT == UNET_LINK_BLOCK && kLinkLdsIds == UNET_LINK_LDS_IDS, "constants of the header");
static_assert(UNET_LINK_COLS == 4 && UNET_LINK_STATUS == 4 && UNET_MATCH_COLS == 4 && UNET_MATCH_STATUS == 5,
              "table layout of the header");
static_assert(kRelabelVecs % RT == 0, "whole rounds of the block");

typedef unsigned long long u64;
enum { COL_FIRST = 0, COL_LAST = 1, COL_PARENT = 2, COL_VOLUME = 3 };
enum { ST_TRACKS = 0, ST_LINKS = 1, ST_DROPPED = 2, ST_OOR = 3 };
enum { M_AREA = 0, M_PARTNER = 1, M_INTER = 2, M_PAREA = 3, MS_DROPPED = 3, MS_OOR = 4 };

// ---- (2) resolve ---------------------------------------------------------------------

// gt_table, pred_table [B][P][M][4] and mstatus [B][P][5] of pass (1), P = max(T - 1, 1);
// lut [B][T][M + 1]; table [B][max_tracks][4]; status [B][4].  lut and table are read
// back by other threads of the block after a barrier: no __restrict__ on them.
__global__ void __launch_bounds__(NT) link_resolve_kernel(const long long* __restrict__ gt_table,
                                                          const long long* __restrict__ pred_table,
                                                          const long long* __restrict__ mstatus, int T, int P, int M,
                                                          int max_tracks, long long num, long long den, int* lut,
                                                          long long* table, long long* __restrict__ status) {
  __shared__ int wsum[2][NT / 64];  // two buffers in turn: one barrier per chunk
  __shared__ u64 red[3];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  gt_table += (size_t)b * P * M * UNET_MATCH_COLS;
  pred_table += (size_t)b * P * M * UNET_MATCH_COLS;
  mstatus += (size_t)b * P * UNET_MATCH_STATUS;
  lut += (size_t)b * T * (M + 1);
  table += (size_t)b * max_tracks * UNET_LINK_COLS;
  for (size_t i = threadIdx.x; i < (size_t)max_tracks * UNET_LINK_COLS; i += NT) table[i] = 0;
  if (threadIdx.x < 3) red[threadIdx.x] = 0;
  __syncthreads();
  long long running = 0;  // tracks so far; < 2^31 (checked by the caller: T min(M, H W) <= INT32_MAX)
  u64 links = 0;
  int round = 0;
  for (int t = 0; t < T; ++t) {
    const long long* mine = t == 0 ? gt_table : pred_table + (size_t)(t - 1) * M * UNET_MATCH_COLS;
    const long long* theirs = gt_table + (size_t)(t > 0 ? t - 1 : 0) * M * UNET_MATCH_COLS;
    const int* prev = lut + (size_t)(t > 0 ? t - 1 : 0) * (M + 1);
    int* cur = lut + (size_t)t * (M + 1);
    for (int c0 = 0; c0 <= M; c0 += NT) {
      const int id = c0 + threadIdx.x;
      long long area = 0, trk = 0, par = 0;
      if (id >= 1 && id <= M) {
        const long long* row = mine + (size_t)(id - 1) * UNET_MATCH_COLS;
        area = row[M_AREA];
        if (area > 0 && t > 0) {
          const long long a = row[M_PARTNER], c = row[M_INTER], aa = row[M_PAREA];
          if (a > 0) {
            if (theirs[(size_t)(a - 1) * UNET_MATCH_COLS + M_PARTNER] == id && c * den > num * (aa + area - c))
              trk = prev[a];
            else if (2 * c > area)
              par = prev[a];
          }
        }
      }
      const bool fresh = area > 0 && trk == 0;
      if (area > 0 && trk != 0) ++links;
      const u64 m = __ballot(fresh);
      const int within = (int)__popcll(m & ((1ull << lane) - 1ull));
      // this chunk's buffer was last read two chunks ago, before the barrier of the chunk between
      int* sums = wsum[round++ & 1];
      if (lane == 0) sums[w] = (int)__popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int j = 0; j < NT / 64; ++j) {
        const int ws = sums[j];
        if (j < w) before += ws;
        total += ws;
      }
      if (fresh) trk = running + before + within + 1;
      running += total;
      if (id <= M) cur[id] = (int)trk;
      if (area > 0 && trk <= max_tracks) {
        long long* row = table + (size_t)(trk - 1) * UNET_LINK_COLS;
        if (fresh) {
          row[COL_FIRST] = t;
          row[COL_PARENT] = par;
        }
        row[COL_LAST] = t;
        row[COL_VOLUME] = (fresh ? 0 : row[COL_VOLUME]) + area;
      }
    }
    __syncthreads();  // cur and the rows are the next frame's input
  }
  u64 dropped = 0, oor = 0;
  for (int p = threadIdx.x; p < P; p += NT) {
    dropped += (u64)mstatus[(size_t)p * UNET_MATCH_STATUS + MS_DROPPED];
    oor += (u64)mstatus[(size_t)p * UNET_MATCH_STATUS + MS_OOR];
  }
  if (links) atomicAdd(&red[0], links);
  if (dropped) atomicAdd(&red[1], dropped);
  if (oor) atomicAdd(&red[2], oor);
  __syncthreads();
  if (threadIdx.x == 0) {
    long long* st = status + (size_t)b * UNET_LINK_STATUS;
    st[ST_TRACKS] = running;
    st[ST_LINKS] = (long long)red[0];
    st[ST_DROPPED] = (long long)red[1];
    st[ST_OOR] = (long long)red[2];
  }
}

// ---- (3) relabel ---------------------------------------------------------------------

__device__ __forceinline__ int look(const int* L, int v, int M) { return (unsigned)v <= (unsigned)M ? L[v] : 0; }

// grid.y = frames; a block takes the 16-byte groups [blockIdx.x kRelabelVecs, + kRelabelVecs)
// of its frame's aligned body.  VEC: labels and out have the same address modulo 16 (the
// host checks it), so one `head` aligns both.  Without VEC every pixel is its own group.
// LDS: the LUT row (M + 1 <= kLinkLdsIds + 1 words) is staged in LDS.
template <bool VEC, bool LDS>
__global__ void __launch_bounds__(RT) link_relabel_kernel(const int* __restrict__ labels, int HW, int M,
                                                          const int* __restrict__ lut, int* __restrict__ out) {
  __shared__ int L[LDS ? kLinkLdsIds + 1 : 1];
  const int n = blockIdx.y;
  const int* row = lut + (size_t)n * (M + 1);
  const size_t base = (size_t)n * (size_t)HW;
  labels += base;
  out += base;
  int head = 0;
  if (VEC) {
    head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(labels) >> 2) & 3u)) & 3u);
    if (head > HW) head = HW;
  }
  const int nvec = VEC ? (HW - head) >> 2 : HW;
  const int v0 = blockIdx.x * kRelabelVecs;
  if (v0 >= nvec && blockIdx.x != 0) return;  // block-uniform, before any barrier
  const int* T = row;  // the table the pixels look up
  if (LDS) {
    for (int i = threadIdx.x; i <= M; i += RT) L[i] = row[i];
    __syncthreads();
    T = L;
  }
  const int v1 = v0 + kRelabelVecs < nvec ? v0 + kRelabelVecs : nvec;
  if (VEC) {
    for (int v = v0 + (int)threadIdx.x; v < v1; v += RT) {
      const int i = head + 4 * v;
      const int4 x = *reinterpret_cast<const int4*>(labels + i);
      int4 o;
      o.x = look(T, x.x, M);
      o.y = look(T, x.y, M);
      o.z = look(T, x.z, M);
      o.w = look(T, x.w, M);
      *reinterpret_cast<int4*>(out + i) = o;
    }
    if (blockIdx.x == 0) {  // at most 3 pixels before the body and 3 after it
      const int tail0 = head + 4 * nvec;
      const int k = (int)threadIdx.x;
      if (k < head) out[k] = look(T, labels[k], M);
      else if (k - head < HW - tail0) out[tail0 + k - head] = look(T, labels[tail0 + k - head], M);
    }
  } else {
    for (int v = v0 + (int)threadIdx.x; v < v1; v += RT) out[v] = look(T, labels[v], M);
  }
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// Workspace: [gt_table | pred_table | mstatus | lut | the workspace of one match call].
// The match workspace is shared by the sequences: their calls follow each other on one
// stream and it holds nothing between calls.
struct Layout {
  size_t gt_table, pred_table, mstatus, lut, match, total;
};
inline int pairs_of(int T) { return T > 1 ? T - 1 : 1; }
inline Layout layout(int B, int T, int M, int max_pairs) {
  const size_t P = (size_t)pairs_of(T);
  Layout l;
  l.gt_table = 0;
  l.pred_table = a256(l.gt_table + (size_t)B * P * M * UNET_MATCH_COLS * 8);
  l.mstatus = a256(l.pred_table + (size_t)B * P * M * UNET_MATCH_COLS * 8);
  l.lut = a256(l.mstatus + (size_t)B * P * UNET_MATCH_STATUS * 8);
  l.match = a256(l.lut + (size_t)B * T * (M + 1) * 4);
  l.total = a256(l.match + (size_t)match_workspace_bytes((int)P, M, M, max_pairs));
  return l;
}

inline bool caps_ok(int B, int T, int M, int max_pairs) {
  return B > 0 && T > 0 && T <= kLinkMaxFrames && (int64_t)B * T <= INT32_MAX && M >= 1 && M <= kMatchMaxId &&
         max_pairs >= 1 && max_pairs <= kMatchMaxPairs;
}

template <bool VEC>
void launch_relabel(bool lds, dim3 grid, hipStream_t st, const int* labels, int HW, int M, const int* lut, int* out) {
  if (lds) link_relabel_kernel<VEC, true><<<grid, dim3(RT), 0, st>>>(labels, HW, M, lut, out);
  else link_relabel_kernel<VEC, false><<<grid, dim3(RT), 0, st>>>(labels, HW, M, lut, out);
}

}  // namespace

int64_t link_workspace_bytes(int B, int T, int max_inst, int max_pairs) {
  if (!caps_ok(B, T, max_inst, max_pairs)) return 0;
  return (int64_t)layout(B, T, max_inst, max_pairs).total;
}

hipError_t launch_link_instances(const LinkArgs& a, hipStream_t st) {
  const int M = a.max_inst;
  if (!a.labels || !a.tracks || a.tracks == a.labels || !a.table || !a.status || !a.workspace ||
      !caps_ok(a.B, a.T, M, a.max_pairs) || a.H <= 0 || a.W <= 0 || a.H > kMeasureMaxDim || a.W > kMeasureMaxDim ||
      (int64_t)a.H * a.W > kMeasureMaxHW || a.max_tracks < 1 || a.iou_den < 1 || a.iou_num < 0 ||
      a.iou_num >= a.iou_den || a.workspace_bytes < link_workspace_bytes(a.B, a.T, M, a.max_pairs))
    return hipErrorInvalidValue;
  const int HW = a.H * a.W;
  // the track ids are int32: at most min(M, H W) new tracks per frame
  if ((int64_t)a.T * (M < HW ? M : HW) > INT32_MAX) return hipErrorInvalidValue;
  const int P = pairs_of(a.T);
  const Layout l = layout(a.B, a.T, M, a.max_pairs);
  char* ws = static_cast<char*>(a.workspace);
  long long* gt_table = reinterpret_cast<long long*>(ws + l.gt_table);
  long long* pred_table = reinterpret_cast<long long*>(ws + l.pred_table);
  long long* mstatus = reinterpret_cast<long long*>(ws + l.mstatus);
  int* lut = reinterpret_cast<int*>(ws + l.lut);
  hipError_t e;
  for (int b = 0; b < a.B; ++b) {
    const int* seq = a.labels + (size_t)b * a.T * HW;
    const MatchArgs m{seq, a.T > 1 ? seq + HW : seq, P, a.H, a.W, M, M, a.max_pairs,
                      gt_table + (size_t)b * P * M * UNET_MATCH_COLS, pred_table + (size_t)b * P * M * UNET_MATCH_COLS,
                      mstatus + (size_t)b * P * UNET_MATCH_STATUS, nullptr, ws + l.match,
                      (int64_t)(l.total - l.match)};
    if ((e = launch_match_instances(m, st)) != hipSuccess) return e;
  }
  for (int b0 = 0; b0 < a.B; b0 += 65535) {
    const unsigned nb = (unsigned)(a.B - b0 < 65535 ? a.B - b0 : 65535);
    link_resolve_kernel<<<dim3(nb), dim3(NT), 0, st>>>(
        gt_table + (size_t)b0 * P * M * UNET_MATCH_COLS, pred_table + (size_t)b0 * P * M * UNET_MATCH_COLS,
        mstatus + (size_t)b0 * P * UNET_MATCH_STATUS, a.T, P, M, a.max_tracks, a.iou_num, a.iou_den,
        lut + (size_t)b0 * a.T * (M + 1), a.table + (size_t)b0 * a.max_tracks * UNET_LINK_COLS,
        a.status + (size_t)b0 * UNET_LINK_STATUS);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const bool vec = ((reinterpret_cast<uintptr_t>(a.labels) ^ reinterpret_cast<uintptr_t>(a.tracks)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.labels) & 3) == 0;
  const bool lds = M <= kLinkLdsIds;
  const int groups = vec ? HW / 4 : HW;  // an upper bound of a frame's 16-byte groups
  const unsigned gx = (unsigned)(groups > 0 ? (groups + kRelabelVecs - 1) / kRelabelVecs : 1);
  const int64_t frames = (int64_t)a.B * a.T;
  for (int64_t n0 = 0; n0 < frames; n0 += 65535) {
    const unsigned nn = (unsigned)(frames - n0 < 65535 ? frames - n0 : 65535);
    const dim3 grid(gx, nn);
    const int* in = a.labels + (size_t)n0 * HW;
    const int* lt = lut + (size_t)n0 * (M + 1);
    int* out = a.tracks + (size_t)n0 * HW;
    if (vec) launch_relabel<true>(lds, grid, st, in, HW, M, lt, out);
    else launch_relabel<false>(lds, grid, st, in, HW, M, lt, out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace unet
