// text.hip — K23 on-device text augmentation (d2r_amd/text_augment.py, --aug_token_delete / --aug_token_mask / --aug_token_replace /
// --aug_whole_word): d2r_token_augment builds the three token tensors of a training batch from their source rows and deletes,
// masks or replaces tokens per sample on the way (the function is stated at its declaration in include/d2r_hip.h).
//
// One wave per output sample, TA_WAVES samples per workgroup, no LDS, no barrier, integer work only.  The wave walks its row in
// chunks of 64 positions, three times (the row is at most 8 KB per tensor and stays in L1 / L2 between the passes):
//   1. n = the number of non-zero mask entries (popcount of a ballot per chunk);
//   2. the effective op of every content position, counted: the keep-one rule needs the number of deleted positions before the
//      first store.  The head of a position is the highest set bit at or below its lane in the ballot of the head flags; its op comes
//      by __shfl from that lane, or from the last head of the earlier chunks (a wave-uniform value carried across chunks);
//   3. the same decisions again, then the stores: a survivor's destination is the running count of survivors plus the popcount of
//      the survivor ballot below its lane.  The tail n'..L-1 is filled with pad_id / 0 / 0.
// Every destination is below n' <= n <= L, every source index below L, and the continuation table is read only at ids inside
// [0, vocab): whatever the device copies of idx / plan hold beyond what the host copies promised, nothing outside the row is touched
// except through idx itself, which the host copy bounds.
#include <algorithm>
#include <utility>

#include "common.h"

namespace {

constexpr int TA_WAVES = 4;  // output samples per 256-thread workgroup

enum : uint32_t { TA_KEEP = 0, TA_DELETE = 1, TA_MASK = 2, TA_REPLACE = 3 };

// The effective op of position l = c0 + lane (content positions only; anything for the others): the op of the plan word of the
// largest head <= l.  `head` / `op` are the lane's own flag and plan op, `carry` the op of the last head of the earlier chunks;
// carry is updated to this chunk's last head.  Executed by all 64 lanes.
__device__ __forceinline__ uint32_t effective_op(bool head, uint32_t op, int lane, uint32_t& carry) {
  const unsigned long long hb = __ballot(head);
  const unsigned long long mine = hb & (~0ull >> (63 - lane));  // heads at or below this lane
  const int src = mine ? 63 - __clzll((long long)mine) : lane;
  const uint32_t from_head = (uint32_t)__shfl((int)op, src, 64);
  const uint32_t eff = mine ? from_head : carry;
  if (hb) carry = (uint32_t)__shfl((int)op, 63 - __clzll((long long)hb), 64);
  return eff;
}

__global__ __launch_bounds__(64 * TA_WAVES) void token_augment_kernel(
    const int64_t* __restrict__ ids, const int64_t* __restrict__ mask, const int64_t* __restrict__ seg, int L,
    const int64_t* __restrict__ idx, const uint32_t* __restrict__ plan, int B, const uint8_t* __restrict__ cont, int64_t vocab,
    int64_t mask_id, int64_t pad_id, int64_t* __restrict__ out_ids, int64_t* __restrict__ out_mask, int64_t* __restrict__ out_seg) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * TA_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;  // a whole wave: no barrier follows
  const int64_t r = idx[b];
  const int64_t* sid = ids + r * L;
  const int64_t* smk = mask + r * L;
  const int64_t* ssg = seg + r * L;
  const uint32_t* pl = plan + (int64_t)b * L;
  int64_t* oid = out_ids + (int64_t)b * L;
  int64_t* omk = out_mask + (int64_t)b * L;
  int64_t* osg = out_seg + (int64_t)b * L;

  int n = 0;
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int l = c0 + lane;
    n += __popcll(__ballot(l < L && smk[l] != 0));
  }
  const int last = n - 2;  // content positions are 1 <= l <= last

  // the decisions of one chunk: the lane's id, plan word and effective op
  auto decide = [&](int l, uint32_t& carry, int64_t& id, uint32_t& word) -> uint32_t {
    const bool content = l >= 1 && l <= last;  // last < L - 1: l is inside the row
    id = l < L ? sid[l] : 0;
    word = l < L ? pl[l] : 0u;
    bool head = false;
    if (content) head = l == 1 || cont == nullptr || id < 0 || id >= vocab || cont[id] == 0;
    return effective_op(head, word & 3u, lane, carry);
  };

  int deleted = 0;
  uint32_t carry = TA_KEEP;
  for (int c0 = 0; c0 <= last; c0 += 64) {
    const int l = c0 + lane;
    int64_t id;
    uint32_t word;
    const uint32_t op = decide(l, carry, id, word);
    deleted += __popcll(__ballot(l >= 1 && l <= last && op == TA_DELETE));
  }
  const bool keep_all = deleted == last;  // every content position deleted: none is (with last <= 0 nothing is content)

  int base = 0;
  carry = TA_KEEP;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int l = c0 + lane;
    int64_t id;
    uint32_t word;
    uint32_t op = decide(l, carry, id, word);
    const bool content = l >= 1 && l <= last;
    if (!content || (keep_all && op == TA_DELETE)) op = TA_KEEP;
    const bool survives = l < n && op != TA_DELETE;
    const unsigned long long sb = __ballot(survives);
    if (survives) {
      const int j = base + __popcll(sb & ~(~0ull << lane));  // survivors below this lane; j <= l < n
      oid[j] = op == TA_MASK ? mask_id : (op == TA_REPLACE ? (int64_t)(word >> 2) : id);
      omk[j] = 1;
      osg[j] = ssg[l];
    }
    base += __popcll(sb);
  }
  for (int j = base + lane; j < L; j += 64) {
    oid[j] = pad_id;
    omk[j] = 0;
    osg[j] = 0;
  }
}

bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int d2r_token_augment(const int64_t* ids, const int64_t* mask, const int64_t* seg, int64_t rows, int L, const int64_t* h_idx,
                                 const int64_t* idx, const uint32_t* h_plan, const uint32_t* plan, int B, const uint8_t* cont,
                                 int64_t vocab, int64_t mask_id, int64_t pad_id, int64_t* out_ids, int64_t* out_mask, int64_t* out_seg,
                                 void* stream) {
  const char* who = "d2r_token_augment";
  D2R_REQUIRE(ids && mask && seg && h_idx && idx && h_plan && plan && out_ids && out_mask && out_seg, "%s: null pointer", who);
  D2R_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d outside [1, 65535]", who, B);
  D2R_REQUIRE(L >= 2 && L <= 1024, "%s: row length %d outside [2, 1024]", who, L);
  D2R_REQUIRE(rows >= 1, "%s: %lld source rows", who, (long long)rows);
  D2R_REQUIRE(vocab >= 1, "%s: vocabulary of %lld ids", who, (long long)vocab);
  D2R_REQUIRE(mask_id >= 0 && mask_id < vocab && pad_id >= 0 && pad_id < vocab, "%s: mask id %lld or pad id %lld outside the %lld ids of the vocabulary",
              who, (long long)mask_id, (long long)pad_id, (long long)vocab);
  for (const void* p : {(const void*)ids, (const void*)mask, (const void*)seg, (const void*)h_idx, (const void*)idx, (const void*)out_ids,
                        (const void*)out_mask, (const void*)out_seg})
    D2R_REQUIRE((reinterpret_cast<uintptr_t>(p) & 7u) == 0, "%s: ids / mask / seg / h_idx / idx / out_* must be 8-byte aligned", who);
  D2R_REQUIRE((reinterpret_cast<uintptr_t>(h_plan) & 3u) == 0 && (reinterpret_cast<uintptr_t>(plan) & 3u) == 0,
              "%s: h_plan / plan must be 4-byte aligned", who);
  for (int b = 0; b < B; ++b)
    D2R_REQUIRE(h_idx[b] >= 0 && h_idx[b] < rows, "%s: index %d is %lld, outside the %lld rows", who, b, (long long)h_idx[b], (long long)rows);
  // whatever the word's own op: a continuation piece is replaced through its head's op by its own id
  for (int64_t k = 0; k < (int64_t)B * L; ++k)
    D2R_REQUIRE((int64_t)(h_plan[k] >> 2) < vocab, "%s: sample %lld, position %lld: replacement id %u outside the %lld ids of the vocabulary",
                who, (long long)(k / L), (long long)(k % L), h_plan[k] >> 2, (long long)vocab);
  const int64_t src_bytes = rows * L * 8, out_bytes = (int64_t)B * L * 8;
  const std::pair<const void*, int64_t> inputs[] = {{ids, src_bytes}, {mask, src_bytes},           {seg, src_bytes},
                                                    {idx, (int64_t)B * 8}, {plan, (int64_t)B * L * 4}, {cont, cont ? vocab : 0}};
  const void* outs[] = {out_ids, out_mask, out_seg};
  for (int o = 0; o < 3; ++o) {
    for (const auto& in : inputs)
      D2R_REQUIRE(in.second == 0 || !overlaps(outs[o], out_bytes, in.first, in.second), "%s: an output overlaps an input tensor", who);
    for (int p = o + 1; p < 3; ++p) D2R_REQUIRE(!overlaps(outs[o], out_bytes, outs[p], out_bytes), "%s: two outputs overlap", who);
  }
  hipLaunchKernelGGL(token_augment_kernel, dim3(d2r_cdiv(B, TA_WAVES)), dim3(64 * TA_WAVES), 0, (hipStream_t)stream, ids, mask, seg, L, idx,
                     plan, B, cont, vocab, mask_id, pad_id, out_ids, out_mask, out_seg);
  return d2r_check_launch(who);
}
