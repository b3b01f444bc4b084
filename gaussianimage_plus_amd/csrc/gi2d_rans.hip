// Payload codings 1 and 2 of the packed stream: the fixed-length records of coding 0, entropy coded (include/gi2d.h
// "rANS payload"; the container table is in INTEGRATION.md), and the two kernels that put a coding-0 payload into
// position order (keys, gather) so that coding 2 has something to gain.
//
// A field of width w is split into hi = v >> lo_bits (the symbol, at most 8 bits) and lo (stored raw).  One CHUNK of
// 2^chunk_log2 records is one wave's work: lane l owns records base + 64 j + l and one 32-bit rANS state (12 probability
// bits, 16-bit renormalisation: a step moves at most one word per lane).  The wave walks j ascending and the coded fields
// ascending; in a step the lanes that need a word take consecutive words of the chunk's shared word stream in ascending
// lane order (__ballot + the popcount of the lanes below).  The encoder runs the same steps backwards.
//
//   histogram  coding-0 payload -> u32[8][256] counts of the hi parts (LDS atomics, one flush per workgroup)
//   encode     coding-0 payload + tables -> per chunk: 64 final states | raw section | words, and its length.  The wave
//              writes its words backwards into LDS and copies the chunk out.  Once per image: not a hot path.
//   expand     coded chunks -> the coding-0 payload, byte for byte.  The hot kernel: several waves per workgroup share the
//              tables in LDS; a chunk (states, raw section, words) is staged into LDS with coalesced loads, so the decode
//              loop has no global load; 64 records (2 R dwords, dword aligned) are ORed together in LDS and leave as
//              coalesced dword stores.
//
// Coding 2 (the DELTA instantiations; `dmask` bit k = field k, k < 2, is differenced): the symbol of a position field is
// the difference of its hi part from the previous record's, mod 2^hb; the first record of a chunk keeps its hi part.  The
// histogram and the encoder also load record g - 1; the expansion undoes the differences with an inclusive wave scan per
// group of 64 records (both fields in one register, 16 bits apart) plus the carry out of the group before.  DELTA = false
// never reads `dmask`: the coding-1 instantiations keep the instructions they had.
//
// Device tables, per coded field in record order (GI2D_RANS_TABLE_BYTES each, built by the host from the stream's
// validated model section): u8 symbol of slot [4096] | u16 cumulative frequency of symbol [258] (entries 256, 257 = 4096).
//
// Every index that comes from stream content is masked or clamped: the slot to 12 bits, the symbol is a byte and indexes
// 258 entries, a word position to the wave's staging area, a chunk's offset and length to the chunk data and the staging
// area.  A stream with nonsense inside decodes to nonsense records inside its own buffers.
#include <vector>

#include "gi2d_batch.h"
#include "gi2d_codec_layout.h"

namespace gi2d {

#define GI2D_RANS_PROB_BITS 12
#define GI2D_RANS_SLOTS (1 << GI2D_RANS_PROB_BITS)
#define GI2D_RANS_LOW 65536u /* states live in [2^16, 2^32) */
#define GI2D_RANS_TABLE_BYTES (GI2D_RANS_SLOTS + 2 * 258)
#define GI2D_RANS_TABLE_DWORDS (GI2D_RANS_TABLE_BYTES / 4)
#define GI2D_RANS_STATIC_LDS (64 * 1024) /* what a launch gets without asking for more */
#define GI2D_RANS_MAX_LDS (160 * 1024)

struct RansLayout {
    CodecLayout rec;
    int lo[GI2D_CODEC_FIELDS];    // raw low bits of a field: max(0, width - 8)
    int rawb[GI2D_CODEC_FIELDS];  // bits of the field in the raw section: lo if coded, the whole width if not
    unsigned mask;                // bit k: field k is entropy coded
    int ncoded;
    int raw_bits;   // R_raw
    int raw_loads;  // dwords a lane's raw bits can touch
    int chunk_log2;
};

static bool rans_layout(const char *what, int kind, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                        int chunk_log2, unsigned mask, RansLayout &L) {
    if (!codec_layout(what, kind, xy_bits, p0_bits, p1_bits, color_bits, L.rec)) return false;
    if (chunk_log2 < 8 || chunk_log2 > 12 || mask > 0xffu) {
        set_error((std::string(what) + ": log2(records per chunk) must be 8..12 and the field mask 8 bits").c_str());
        return false;
    }
    L.mask = mask;
    L.chunk_log2 = chunk_log2;
    L.ncoded = L.raw_bits = 0;
    for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
        const int w = L.rec.width[k];
        L.lo[k] = w > 8 ? w - 8 : 0;
        const bool coded = (mask >> k) & 1u;
        L.rawb[k] = coded ? L.lo[k] : w;
        L.ncoded += coded;
        L.raw_bits += L.rawb[k];
    }
    L.raw_loads = L.raw_bits ? (31 + L.raw_bits + 31) / 32 : 0;
    return true;
}
static inline int rans_chunks(long long n, int chunk_log2) { return (int)((n + (1ll << chunk_log2) - 1) >> chunk_log2); }
// dwords of a full chunk's raw section / most words a chunk can hold / dwords of the largest chunk
static inline int rans_raw_cap(const RansLayout &L) { return ((L.raw_bits << L.chunk_log2) + 31) / 32; }
static inline int rans_word_cap(const RansLayout &L) { return L.ncoded << L.chunk_log2; }
static inline int rans_chunk_cap(const RansLayout &L) { return 64 + rans_raw_cap(L) + (rans_word_cap(L) + 1) / 2; }

// The lanes of ONE wave hand data to each other through LDS here.  LDS operations of a wave complete in order, so all
// this has to do is keep the compiler from moving them across the point -- and it must not wait for the global stores
// in flight, which a workgroup-scope fence does (the flush of 64 records would cost a store round trip per group).
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Record g of a coding-0 payload as a 128-bit little-endian number (the load of codec_decode_bin_kernel).
__device__ __forceinline__ void rans_load_record(const uint32_t *__restrict__ payload, long long g,
                                                 const CodecLayout &lay, long long last_dword, uint32_t (&r)[4]) {
    const long long bit0 = g * lay.record_bits;
    const long long first = bit0 >> 5;
    uint32_t w[GI2D_CODEC_MAX_LOADS];
#pragma unroll
    for (int j = 0; j < GI2D_CODEC_MAX_LOADS; ++j) {
        const long long d = first + j;
        w[j] = j < lay.loads ? payload[d < last_dword ? d : last_dword] : 0u;
    }
    const uint32_t s0 = (uint32_t)bit0 & 31u;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_alignbit(w[j + 1], w[j], s0);
}

// Appends the w-bit value v (1 <= w <= 16) to a record that grows down from bit 127 ...
__device__ __forceinline__ void rans_push(uint32_t (&r)[4], uint32_t v, int w) {
    r[0] = __builtin_amdgcn_alignbit(r[1], r[0], (uint32_t)w);
    r[1] = __builtin_amdgcn_alignbit(r[2], r[1], (uint32_t)w);
    r[2] = __builtin_amdgcn_alignbit(r[3], r[2], (uint32_t)w);
    r[3] = (r[3] >> w) | (v << (32 - w));
}
// ... and moves the `bits` bits pushed so far down to bit 0.
__device__ __forceinline__ void rans_settle(uint32_t (&r)[4], int bits) {
    int sh = 128 - bits;
    for (; sh >= 32; sh -= 32) r[0] = r[1], r[1] = r[2], r[2] = r[3], r[3] = 0u;
    r[0] = __builtin_amdgcn_alignbit(r[1], r[0], (uint32_t)sh);
    r[1] = __builtin_amdgcn_alignbit(r[2], r[1], (uint32_t)sh);
    r[2] = __builtin_amdgcn_alignbit(r[3], r[2], (uint32_t)sh);
    r[3] >>= sh;
}
// ORs the 128-bit number r into the LDS dwords `area[0, area_dwords)` at bit position `bit`.
__device__ __forceinline__ void rans_or_into(uint32_t *area, int area_dwords, int bit, const uint32_t (&r)[4]) {
    const int d0 = bit >> 5, s = bit & 31;
    uint32_t prev = 0u;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint32_t cur = i < 4 ? r[i] : 0u;
        const uint32_t e = (uint32_t)(((((uint64_t)cur << 32) | prev) << s) >> 32);
        if (e != 0u && d0 + i < area_dwords) atomicOr(&area[d0 + i], e);
        prev = cur;
    }
}

// ------------------------------------------------------------------------------------------------------ histogram
template <bool DELTA>
__global__ __launch_bounds__(256) void rans_histogram_kernel(int n, RansLayout L, const uint32_t *__restrict__ payload,
                                                             long long last_dword, uint32_t *__restrict__ hist,
                                                             unsigned dmask) {
    __shared__ uint32_t h[GI2D_CODEC_FIELDS * 256];
    const int tid = threadIdx.x;
    for (int i = tid; i < GI2D_CODEC_FIELDS * 256; i += 256) h[i] = 0u;
    __syncthreads();
    for (long long g = (long long)blockIdx.x * 256 + tid; g < n; g += (long long)gridDim.x * 256) {
        uint32_t r[4];
        rans_load_record(payload, g, L.rec, last_dword, r);
        uint32_t prev[2] = {0u, 0u};  // DELTA: hi parts of the position fields of record g - 1 (0 at the start of a chunk)
        if (DELTA && (g & ((1ll << L.chunk_log2) - 1)) != 0) {
            uint32_t q[4];
            rans_load_record(payload, g - 1, L.rec, last_dword, q);
            prev[0] = codec_take(q, L.rec.width[0]) >> L.lo[0];
            prev[1] = codec_take(q, L.rec.width[1]) >> L.lo[1];
        }
#pragma unroll
        for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
            const uint32_t v = codec_take(r, L.rec.width[k]);
            uint32_t s = (v >> L.lo[k]) & 255u;
            if (DELTA && k < 2 && ((dmask >> k) & 1u)) s = (s - prev[k]) & ((1u << (L.rec.width[k] - L.lo[k])) - 1u);
            atomicAdd(&h[k * 256 + s], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < GI2D_CODEC_FIELDS * 256; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// --------------------------------------------------------------------------------------------------------- encode
struct RansEncodeArgs {
    RansLayout L;
    int n;
    const uint32_t *payload;  // coding 0
    long long last_dword;
    const uint16_t *tables;   // device tables (only the cumulative frequencies are read)
    uint32_t *out;            // chunk c at dword c * stride
    int stride, raw_cap, word_cap;
    uint32_t *lengths;        // bytes of chunk c; 0xffffffff: a symbol of frequency 0 (tables of another payload)
    unsigned dmask;           // DELTA only: the differenced fields
};

template <bool DELTA>
__global__ __launch_bounds__(64) void rans_encode_kernel(RansEncodeArgs a) {
    extern __shared__ __align__(16) uint32_t lds[];
    const int lane = threadIdx.x, c = blockIdx.x;
    uint32_t *raw = lds;
    uint16_t *words = (uint16_t *)(lds + a.raw_cap);
    const int crec = 1 << a.L.chunk_log2;
    const long long base = (long long)c * crec;
    const int records = (int)min((long long)crec, (long long)a.n - base);
    const int raw_dw = (records * a.L.raw_bits + 31) >> 5;
    for (int i = lane; i < raw_dw; i += 64) raw[i] = 0u;
    wave_lds_sync();
    uint32_t x = GI2D_RANS_LOW;
    int wend = a.word_cap;
    bool bad = false;
    for (int j = ((records + 63) >> 6) - 1; j >= 0; --j) {
        const int rl = j * 64 + lane;
        const bool active = rl < records;
        uint32_t r[4], v[GI2D_CODEC_FIELDS];
        rans_load_record(a.payload, active ? base + rl : base, a.L.rec, a.last_dword, r);
        uint32_t rr[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
            v[k] = codec_take(r, a.L.rec.width[k]);
            if (a.L.rawb[k]) rans_push(rr, v[k] & ((1u << a.L.rawb[k]) - 1u), a.L.rawb[k]);
        }
        if (a.L.raw_bits && active) {
            rans_settle(rr, a.L.raw_bits);
            rans_or_into(raw, raw_dw, rl * a.L.raw_bits, rr);
        }
        uint32_t prev[2] = {0u, 0u};  // DELTA: hi parts of the position fields of the record before (0 for the chunk's first)
        if (DELTA) {
            uint32_t q[4];
            rans_load_record(a.payload, active && rl > 0 ? base + rl - 1 : base, a.L.rec, a.last_dword, q);
            const uint32_t p0 = codec_take(q, a.L.rec.width[0]) >> a.L.lo[0];
            const uint32_t p1 = codec_take(q, a.L.rec.width[1]) >> a.L.lo[1];
            if (rl > 0) prev[0] = p0, prev[1] = p1;
        }
#pragma unroll
        for (int k = GI2D_CODEC_FIELDS - 1; k >= 0; --k) {
            if (!((a.L.mask >> k) & 1u)) continue;
            const int t = __popc(a.L.mask & ((1u << k) - 1u));
            const uint16_t *cum = a.tables + t * (GI2D_RANS_TABLE_BYTES / 2) + GI2D_RANS_SLOTS / 2;
            uint32_t s = (v[k] >> a.L.lo[k]) & 255u;
            if (DELTA && k < 2 && ((a.dmask >> k) & 1u)) s = (s - prev[k]) & ((1u << (a.L.rec.width[k] - a.L.lo[k])) - 1u);
            const uint32_t c0 = cum[s];
            uint32_t f = (uint32_t)cum[s + 1] - c0;
            if (active && (f == 0u || f > GI2D_RANS_SLOTS)) bad = true;
            if (f == 0u || f > GI2D_RANS_SLOTS) f = 1u;
            const bool emit = active && (uint64_t)x >= ((uint64_t)f << 20);
            const unsigned long long m = __ballot(emit);
            const int cnt = __popcll(m);
            if (emit) {
                const int p = wend - cnt + __popcll(m & lanemask_lt());
                if (p >= 0) words[p] = (uint16_t)(x & 0xffffu);
                x >>= 16;
            }
            wend = max(wend - cnt, 0);
            if (active) x = ((x / f) << 12) + x % f + c0;
        }
    }
    wave_lds_sync();
    const int nwords = a.word_cap - wend;
    uint32_t *out = a.out + (long long)c * a.stride;
    out[lane] = x;
    for (int i = lane; i < raw_dw; i += 64) out[64 + i] = raw[i];
    const int wdw = (nwords + 1) >> 1;
    for (int i = lane; i < wdw; i += 64) {
        const uint32_t lo = words[wend + 2 * i];
        const uint32_t hi = 2 * i + 1 < nwords ? words[wend + 2 * i + 1] : 0u;
        out[64 + raw_dw + i] = lo | (hi << 16);
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) a.lengths[c] = any_bad ? 0xffffffffu : 4u * (uint32_t)(64 + raw_dw + wdw);
}

// --------------------------------------------------------------------------------------------------------- expand
struct RansExpandArgs {
    RansLayout L;
    int n, chunks;
    const uint32_t *tables;  // ncoded * GI2D_RANS_TABLE_DWORDS
    const uint32_t *dir;     // chunks + 1 byte offsets into the chunk data
    const uint32_t *data;
    uint32_t data_dwords;
    int in_cap;              // dwords of a wave's staging area (>= the largest chunk)
    uint32_t *out;           // coding-0 payload
    long long out_dwords;
    int32_t *status;         // raised to `token` if an active lane does not end at 2^16
    int token;
    unsigned dmask;          // DELTA only: the differenced fields
};

// The work of one workgroup of the expansion: the tables of the stream `a` into LDS, then wave w expands chunk
// block * waves + w of that stream (a wave past the stream's last chunk idles).  Called by every thread of the workgroup
// (it holds the workgroup's one barrier); `lds`: a.L.ncoded tables + waves * (a.in_cap + 2 R) dwords.
template <bool DELTA>
__device__ __forceinline__ void rans_expand_block(const RansExpandArgs &a, uint32_t *lds, int block) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int table_dw = a.L.ncoded * GI2D_RANS_TABLE_DWORDS;
    for (int i = tid; i < table_dw; i += blockDim.x) lds[i] = a.tables[i];
    const int R = a.L.rec.record_bits, group_dw = 2 * R;  // 64 records: dword aligned
    uint32_t *in = lds + table_dw + wave * (a.in_cap + group_dw);
    uint32_t *grp = in + a.in_cap;
    const int c = block * waves + wave;
    if (c < a.chunks) {
        // the chunk: states | raw section | words, as it lies in the stream
        const uint32_t o0 = min(a.dir[c] >> 2, a.data_dwords), o1 = min(a.dir[c + 1] >> 2, a.data_dwords);
        const uint32_t len = o1 > o0 ? min(o1 - o0, (uint32_t)a.in_cap) : 0u;
        for (uint32_t i = lane; i < len; i += 64) in[i] = a.data[o0 + i];
        for (int i = lane; i < group_dw; i += 64) grp[i] = 0u;
    }
    __syncthreads();
    if (c >= a.chunks) return;
    const int crec = 1 << a.L.chunk_log2;
    const long long base = (long long)c * crec;
    const int records = (int)min((long long)crec, (long long)a.n - base);
    const int raw_dw = (records * a.L.raw_bits + 31) >> 5;
    const int last_in = a.in_cap - 1, last_word = 2 * a.in_cap - 1;
    const uint16_t *in16 = (const uint16_t *)in;
    const uint8_t *tab8 = (const uint8_t *)lds;
    const uint16_t *tab16 = (const uint16_t *)lds;
    uint32_t x = in[lane];
    int wpos = 2 * (64 + raw_dw);  // u16 index of the next word
    const unsigned long long below = lanemask_lt();
    const long long out_base = (base * R) >> 5;
    const int J = (records + 63) >> 6;
    // DELTA: the hi parts of the position fields of the record before this group, field 0 in bits 0..15, field 1 in
    // bits 16..31 (0 in front of the chunk's first record); wave uniform
    uint32_t carry = 0u;
    for (int j = 0; j < J; ++j) {
        const int rl = j * 64 + lane;
        const bool active = rl < records;
        uint32_t r[4] = {0u, 0u, 0u, 0u};
        if (a.L.raw_bits) {
            const int bit0 = rl * a.L.raw_bits, first = 64 + (bit0 >> 5);
            uint32_t w[GI2D_CODEC_MAX_LOADS];
#pragma unroll
            for (int q = 0; q < GI2D_CODEC_MAX_LOADS; ++q) w[q] = q < a.L.raw_loads ? in[min(first + q, last_in)] : 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = __builtin_amdgcn_alignbit(w[q + 1], w[q], (uint32_t)bit0 & 31u);
        }
        uint32_t rec[4] = {0u, 0u, 0u, 0u};
        uint32_t diff = 0u, v0 = 0u;  // DELTA: the lane's differenced symbols, packed like `carry`; field 0 waits for field 1
#pragma unroll
        for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
            const int w = a.L.rec.width[k];
            uint32_t v;
            if ((a.L.mask >> k) & 1u) {
                const int t = __popc(a.L.mask & ((1u << k) - 1u));
                const uint32_t slot = x & (GI2D_RANS_SLOTS - 1u);
                const uint32_t s = tab8[t * GI2D_RANS_TABLE_BYTES + slot];
                const uint16_t *cum = tab16 + t * (GI2D_RANS_TABLE_BYTES / 2) + GI2D_RANS_SLOTS / 2;
                const uint32_t c0 = cum[s], c1 = cum[s + 1];
                uint32_t xn = (c1 - c0) * (x >> GI2D_RANS_PROB_BITS) + slot - c0;
                const bool need = active && xn < GI2D_RANS_LOW;
                // (no branch around the word read: with 64 lanes some lane needs a word in nearly every step)
                const unsigned long long m = __ballot(need);
                const uint32_t word = in16[min(wpos + (int)__popcll(m & below), last_word)];
                wpos += __popcll(m);
                x = need ? (xn << 16) | word : active ? xn : x;
                v = (s << a.L.lo[k]) | codec_take(r, a.L.lo[k]);
                // lanes past the last record add nothing to the scan
                if (DELTA && k < 2 && ((a.dmask >> k) & 1u) && active) diff |= s << (16 * k);
            } else {
                v = codec_take(r, w);
            }
            if (DELTA && k == 0) {
                v0 = v;
                continue;
            }
            if (DELTA && k == 1) {
                // inclusive scan of the 64 lanes' symbols (a sum stays below 64 * 255 + 255: the halves do not meet), the
                // carry of the group before, every hi part mod 2^hb; outside any lane-divergent branch
                uint32_t t = diff;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(t, d);
                    t += lane >= d ? up : 0u;
                }
                t += carry;
                const uint32_t hbm = (1u << (w - a.L.lo[1])) - 1u, lom = (1u << a.L.lo[1]) - 1u;  // fields 0 and 1: one width
                carry = (uint32_t)__builtin_amdgcn_readlane((int)t, 63) & (hbm | (hbm << 16));
                if (a.dmask & 1u) v0 = ((t & hbm) << a.L.lo[0]) | (v0 & lom);
                if (a.dmask & 2u) v = (((t >> 16) & hbm) << a.L.lo[1]) | (v & lom);
                rans_push(rec, v0 & ((1u << w) - 1u), w);
            }
            rans_push(rec, v & ((1u << w) - 1u), w);
        }
        rans_settle(rec, R);
        if (active) rans_or_into(grp, group_dw, lane * R, rec);
        wave_lds_sync();
        const long long gd0 = out_base + (long long)j * group_dw;
        for (int i = lane; i < group_dw; i += 64) {
            const uint32_t d = grp[i];
            grp[i] = 0u;
            if (gd0 + i < a.out_dwords) a.out[gd0 + i] = d;
        }
        wave_lds_sync();
    }
    const bool bad = lane < records && x != GI2D_RANS_LOW;
    if (__ballot(bad) != 0ull && lane == 0) atomicMax(a.status, a.token);
}

template <bool DELTA>
__global__ __launch_bounds__(256) void rans_expand_kernel(RansExpandArgs a) {
    extern __shared__ __align__(16) uint32_t lds[];
    rans_expand_block<DELTA>(a, lds, (int)blockIdx.x);
}

// Several streams per expansion launch (include/gi2d.h gi2d_codec_rans_expand_batch; DESIGN.md 3.8 "Batched expansion"):
// the device table is a head -- the workgroup at which stream s starts -- and one argument block per stream, written as
// gi2d_codec_batch.hip writes its table.  A workgroup finds its stream with batch_find and does that stream's work only:
// its tables, its chunks, its output range and its status word; the last workgroup of a stream leaves its surplus waves
// idle.  DELTA is a workgroup-uniform branch here.
struct RansBatchHead {
    int wg_start[96];  // GI2D_BATCH_MAX + 1 used; entry K = number of workgroups
};
struct RansBatchTable {
    RansBatchHead *head;
    RansExpandArgs *args;
    size_t bytes;
};
static inline size_t rans_batch_bytes(int k) {
    return align_up(sizeof(RansBatchHead)) + (size_t)(k > 0 ? k : 1) * sizeof(RansExpandArgs);
}
static inline RansBatchTable carve_rans_batch(void *base, int k) {  // base: not null
    RansBatchTable b;
    b.head = (RansBatchHead *)base;
    b.args = (RansExpandArgs *)((char *)base + align_up(sizeof(RansBatchHead)));
    b.bytes = rans_batch_bytes(k);
    return b;
}
#define GI2D_RANS_BATCH_PACK 16 /* argument blocks per writer launch (kernel arguments are limited to 4 KB) */
struct RansBatchPack {
    RansExpandArgs args[GI2D_RANS_BATCH_PACK];
};
static_assert(sizeof(RansBatchPack) <= 3840 && sizeof(RansBatchHead) <= 3840,
              "a writer's block must fit the kernel-argument segment");

__global__ __launch_bounds__(256) void rans_expand_batched_kernel(const RansBatchHead *__restrict__ head,
                                                                  const RansExpandArgs *__restrict__ args, int k_streams) {
    extern __shared__ __align__(16) uint32_t lds[];
    const int s = batch_find(head->wg_start, k_streams, (int)blockIdx.x);
    const RansExpandArgs a = args[s];
    const int block = (int)blockIdx.x - head->wg_start[s];
    if (a.dmask)  // workgroup-uniform
        rans_expand_block<true>(a, lds, block);
    else
        rans_expand_block<false>(a, lds, block);
}

// ------------------------------------------------------------------------------------------------- position order
// The position key of every record of a coding-0 payload: hi(y) * 2^hb + hi(x), the hi parts as the coder splits them.
__global__ __launch_bounds__(256) void codec_position_keys_kernel(int n, RansLayout L, const uint32_t *__restrict__ payload,
                                                                  long long last_dword, int32_t *__restrict__ keys) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    uint32_t r[4];
    rans_load_record(payload, g, L.rec, last_dword, r);
    const uint32_t x = codec_take(r, L.rec.width[0]) >> L.lo[0];
    const uint32_t y = codec_take(r, L.rec.width[1]) >> L.lo[1];
    keys[g] = (int32_t)((y << (L.rec.width[0] - L.lo[0])) | x);
}

// Record g of `out` = record perm[g] of `payload`.  Built like the pack kernel: the 256 records of a workgroup are
// exactly 8 R dwords and start dword aligned, so they are ORed together in LDS and leave as coalesced dword stores --
// every output dword, the zero padding behind the last record included, is written exactly once.
__global__ __launch_bounds__(GI2D_CODEC_PACK_BLOCK) void codec_gather_kernel(
    int n, CodecLayout lay, const uint32_t *__restrict__ payload, long long last_dword, const int32_t *__restrict__ perm,
    uint32_t *__restrict__ out, long long total_dwords) {
    __shared__ uint32_t grp[GI2D_CODEC_PACK_BLOCK * GI2D_CODEC_MAX_RECORD / 32];
    const int tid = threadIdx.x;
    const int group_dwords = GI2D_CODEC_PACK_BLOCK / 32 * lay.record_bits;
    for (int i = tid; i < group_dwords; i += GI2D_CODEC_PACK_BLOCK) grp[i] = 0u;
    __syncthreads();
    const long long g = (long long)blockIdx.x * GI2D_CODEC_PACK_BLOCK + tid;
    if (g < n) {
        const int src = min(max(perm[g], 0), n - 1);  // an index from a caller's array: clamped before it forms an address
        uint32_t r[4];
        rans_load_record(payload, src, lay, last_dword, r);
        // the load brings the start of the next record along: keep R bits
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int keep = lay.record_bits - 32 * j;
            r[j] = keep >= 32 ? r[j] : keep > 0 ? r[j] & ((1u << keep) - 1u) : 0u;
        }
        rans_or_into(grp, group_dwords, tid * lay.record_bits, r);
    }
    __syncthreads();
    const long long base = (long long)blockIdx.x * group_dwords;
    for (int i = tid; i < group_dwords; i += GI2D_CODEC_PACK_BLOCK)
        if (base + i < total_dwords) out[base + i] = grp[i];
}

// A launch that needs more than 64 KB of LDS asks for it first (a CU has 160 KB).
template <typename K>
static bool rans_reserve_lds(const char *what, K kernel, size_t bytes) {
    if (bytes <= GI2D_RANS_STATIC_LDS) return true;
    if (bytes > GI2D_RANS_MAX_LDS ||
        hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error((std::string(what) + ": the chunk does not fit the LDS of a compute unit").c_str());
        return false;
    }
    return true;
}

static int rans_fail(const char *what, const char *why, int rc) {
    set_error((std::string(what) + ": " + why).c_str());
    return rc;
}
// Only the position fields can be differenced, and a differenced field is a coded field.
static bool rans_delta_mask_ok(const char *what, unsigned coded_mask, unsigned delta_mask) {
    if ((delta_mask & ~3u) || (delta_mask & ~coded_mask)) {
        rans_fail(what, "only the coded fields among 0 and 1 can be differenced", GI2D_ERR_INVALID_ARGUMENT);
        return false;
    }
    return true;
}

// The entries of coding 1 and coding 2 share their checks and launches; delta_mask = 0 takes the coding-1 kernels.
static int rans_histogram(const char *what, int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                          int chunk_log2, unsigned delta_mask, const void *payload, size_t payload_bytes, uint32_t *hist,
                          gi2d_stream_t st) {
    RansLayout L;
    if (!rans_layout(what, kind, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, 0u, L)) return GI2D_ERR_INVALID_ARGUMENT;
    if (!rans_delta_mask_ok(what, 3u, delta_mask)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 0) return rans_fail(what, "negative size", GI2D_ERR_INVALID_ARGUMENT);
    const long long need = codec_dwords(n, L.rec.record_bits);
    if (payload_bytes < (size_t)need * 4)
        return rans_fail(what, "payload shorter than 4 * ceil(N * R / 32) bytes", GI2D_ERR_INVALID_ARGUMENT);
    if (!hist || ((uintptr_t)hist & 3) || (n > 0 && (!payload || ((uintptr_t)payload & 3))))
        return rans_fail(what, "null or misaligned pointer", GI2D_ERR_INVALID_ARGUMENT);
    hipError_t e = hipMemsetAsync(hist, 0, GI2D_CODEC_FIELDS * 256 * sizeof(uint32_t), (hipStream_t)st);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return GI2D_OK;
    const int groups = (n + 255) / 256;
    const dim3 grid(groups < 256 ? groups : 256), block(256);
    if (delta_mask)
        hipLaunchKernelGGL(rans_histogram_kernel<true>, grid, block, 0, (hipStream_t)st, n, L, (const uint32_t *)payload,
                           need - 1, hist, delta_mask);
    else
        hipLaunchKernelGGL(rans_histogram_kernel<false>, grid, block, 0, (hipStream_t)st, n, L, (const uint32_t *)payload,
                           need - 1, hist, 0u);
    return check_launch(what);
}

static int rans_encode(const char *what, int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                       int chunk_log2, unsigned coded_mask, unsigned delta_mask, const void *tables, size_t tables_bytes,
                       const void *payload, size_t payload_bytes, void *scratch, size_t scratch_bytes, uint32_t *lengths,
                       gi2d_stream_t st) {
    RansLayout L;
    if (!rans_layout(what, kind, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask, L))
        return GI2D_ERR_INVALID_ARGUMENT;
    if (!rans_delta_mask_ok(what, coded_mask, delta_mask)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 1) return rans_fail(what, "no gaussians", GI2D_ERR_INVALID_ARGUMENT);
    const long long need = codec_dwords(n, L.rec.record_bits);
    const int chunks = rans_chunks(n, chunk_log2), stride = rans_chunk_cap(L);
    if (payload_bytes < (size_t)need * 4 || tables_bytes != (size_t)L.ncoded * GI2D_RANS_TABLE_BYTES)
        return rans_fail(what, "payload shorter than 4 * ceil(N * R / 32) bytes, or tables not one per coded field",
                         GI2D_ERR_INVALID_ARGUMENT);
    if (scratch_bytes < (size_t)chunks * stride * 4)
        return rans_fail(what, "scratch smaller than gi2d_codec_rans_scratch_bytes", GI2D_ERR_WORKSPACE_TOO_SMALL);
    if (!payload || !scratch || !lengths || (L.ncoded && !tables) || (((uintptr_t)payload | (uintptr_t)scratch |
                                                                       (uintptr_t)lengths | (uintptr_t)tables) & 3))
        return rans_fail(what, "null or misaligned pointer", GI2D_ERR_INVALID_ARGUMENT);
    RansEncodeArgs a;
    a.L = L, a.n = n, a.payload = (const uint32_t *)payload, a.last_dword = need - 1;
    a.tables = (const uint16_t *)tables, a.out = (uint32_t *)scratch, a.stride = stride;
    a.raw_cap = rans_raw_cap(L), a.word_cap = rans_word_cap(L), a.lengths = lengths, a.dmask = delta_mask;
    const size_t lds = (size_t)a.raw_cap * 4 + (size_t)a.word_cap * 2 + 16;
    if (delta_mask) {
        if (!rans_reserve_lds(what, rans_encode_kernel<true>, lds)) return GI2D_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(rans_encode_kernel<true>, dim3(chunks), dim3(64), lds, (hipStream_t)st, a);
    } else {
        if (!rans_reserve_lds(what, rans_encode_kernel<false>, lds)) return GI2D_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(rans_encode_kernel<false>, dim3(chunks), dim3(64), lds, (hipStream_t)st, a);
    }
    return check_launch(what);
}

// The checks of one stream's expansion, shared by the single entries and the batched one -> its argument block and the
// two LDS footprints a launch is sized by: the tables' bytes and one wave's (staging area + the group of 64 records).
static int rans_expand_args(const char *what, int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                            int chunk_log2, unsigned coded_mask, unsigned delta_mask, const void *tables,
                            size_t tables_bytes, const void *directory, const void *chunk_data, size_t chunk_data_bytes,
                            size_t max_chunk_bytes, void *payload, size_t payload_bytes, int32_t *status, int token,
                            RansExpandArgs &a, size_t &table_b, size_t &wave_b) {
    RansLayout L;
    if (!rans_layout(what, kind, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask, L))
        return GI2D_ERR_INVALID_ARGUMENT;
    if (!rans_delta_mask_ok(what, coded_mask, delta_mask)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 1) return rans_fail(what, "no gaussians", GI2D_ERR_INVALID_ARGUMENT);
    const long long need = codec_dwords(n, L.rec.record_bits);
    const int chunks = rans_chunks(n, chunk_log2);
    if (payload_bytes < (size_t)need * 4 || tables_bytes != (size_t)L.ncoded * GI2D_RANS_TABLE_BYTES)
        return rans_fail(what, "output shorter than 4 * ceil(N * R / 32) bytes, or tables not one per coded field",
                         GI2D_ERR_INVALID_ARGUMENT);
    // every chunk holds its states and raw section; none is longer than the largest the coder can make
    const int full = 64 + rans_raw_cap(L);
    const int tail_records = n - ((chunks - 1) << chunk_log2);
    const int smallest = chunks > 1 ? full : 64 + (tail_records * L.raw_bits + 31) / 32;
    if ((max_chunk_bytes & 3) || max_chunk_bytes < (size_t)smallest * 4 || max_chunk_bytes > (size_t)rans_chunk_cap(L) * 4 ||
        (chunk_data_bytes & 3) || chunk_data_bytes > 0xffffffffull || chunk_data_bytes < max_chunk_bytes)
        return rans_fail(what, "chunk sizes do not fit N, the field widths and the chunk size", GI2D_ERR_INVALID_ARGUMENT);
    if (!directory || !chunk_data || !payload || !status || (L.ncoded && !tables) ||
        (((uintptr_t)directory | (uintptr_t)chunk_data | (uintptr_t)payload | (uintptr_t)status | (uintptr_t)tables) & 3))
        return rans_fail(what, "null or misaligned pointer", GI2D_ERR_INVALID_ARGUMENT);
    a.L = L, a.n = n, a.chunks = chunks, a.tables = (const uint32_t *)tables, a.dir = (const uint32_t *)directory;
    a.data = (const uint32_t *)chunk_data, a.data_dwords = (uint32_t)(chunk_data_bytes / 4);
    a.in_cap = (int)(max_chunk_bytes / 4), a.out = (uint32_t *)payload, a.out_dwords = need;
    a.status = status, a.token = token, a.dmask = delta_mask;
    table_b = (size_t)L.ncoded * GI2D_RANS_TABLE_BYTES;
    wave_b = ((size_t)a.in_cap + 2 * L.rec.record_bits) * 4;
    return GI2D_OK;
}
// Waves per workgroup of an expansion launch: as many of 4 as share the tables within the LDS a launch gets without
// asking, and no more than the launch has chunks for (`chunks`: of its stream, or of its largest stream).
static int rans_expand_waves(size_t table_b, size_t wave_b, int chunks) {
    int waves = 4;
    while (waves > 1 && (table_b + waves * wave_b > GI2D_RANS_STATIC_LDS || waves > chunks)) waves >>= 1;
    return waves;
}

static int rans_expand(const char *what, int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                       int chunk_log2, unsigned coded_mask, unsigned delta_mask, const void *tables, size_t tables_bytes,
                       const void *directory, const void *chunk_data, size_t chunk_data_bytes, size_t max_chunk_bytes,
                       void *payload, size_t payload_bytes, int32_t *status, int token, gi2d_stream_t st) {
    RansExpandArgs a;
    size_t table_b, wave_b;
    const int rc = rans_expand_args(what, kind, n, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask, delta_mask,
                                    tables, tables_bytes, directory, chunk_data, chunk_data_bytes, max_chunk_bytes, payload,
                                    payload_bytes, status, token, a, table_b, wave_b);
    if (rc != GI2D_OK) return rc;
    const int chunks = a.chunks, waves = rans_expand_waves(table_b, wave_b, chunks);
    const size_t lds = table_b + waves * wave_b;
    const dim3 grid((chunks + waves - 1) / waves), block(64 * waves);
    if (delta_mask) {
        if (!rans_reserve_lds(what, rans_expand_kernel<true>, lds)) return GI2D_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(rans_expand_kernel<true>, grid, block, lds, (hipStream_t)st, a);
    } else {
        if (!rans_reserve_lds(what, rans_expand_kernel<false>, lds)) return GI2D_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(rans_expand_kernel<false>, grid, block, lds, (hipStream_t)st, a);
    }
    return check_launch(what);
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

size_t gi2d_codec_rans_scratch_bytes(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                                     int chunk_log2, unsigned coded_mask) {
    RansLayout L;
    if (n < 0 || !rans_layout("codec rans scratch bytes", kind, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2,
                              coded_mask, L))
        return 0;
    return (size_t)rans_chunks(n, chunk_log2) * rans_chunk_cap(L) * 4;
}

int gi2d_codec_histogram(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, const void *payload,
                         size_t payload_bytes, uint32_t *hist, gi2d_stream_t st) {
    return rans_histogram("codec histogram", kind, n, xy_bits, p0_bits, p1_bits, color_bits, 8, 0u, payload,
                          payload_bytes, hist, st);
}

int gi2d_codec_histogram_delta(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, int chunk_log2,
                               unsigned delta_mask, const void *payload, size_t payload_bytes, uint32_t *hist,
                               gi2d_stream_t st) {
    return rans_histogram("codec histogram delta", kind, n, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, delta_mask,
                          payload, payload_bytes, hist, st);
}

int gi2d_codec_rans_encode(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, int chunk_log2,
                           unsigned coded_mask, const void *tables, size_t tables_bytes, const void *payload,
                           size_t payload_bytes, void *scratch, size_t scratch_bytes, uint32_t *lengths,
                           gi2d_stream_t st) {
    return rans_encode("codec rans encode", kind, n, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask, 0u,
                       tables, tables_bytes, payload, payload_bytes, scratch, scratch_bytes, lengths, st);
}

int gi2d_codec_rans_encode_delta(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, int chunk_log2,
                                 unsigned coded_mask, unsigned delta_mask, const void *tables, size_t tables_bytes,
                                 const void *payload, size_t payload_bytes, void *scratch, size_t scratch_bytes,
                                 uint32_t *lengths, gi2d_stream_t st) {
    return rans_encode("codec rans encode delta", kind, n, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask,
                       delta_mask, tables, tables_bytes, payload, payload_bytes, scratch, scratch_bytes, lengths, st);
}

int gi2d_codec_rans_expand(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, int chunk_log2,
                           unsigned coded_mask, const void *tables, size_t tables_bytes, const void *directory,
                           const void *chunk_data, size_t chunk_data_bytes, size_t max_chunk_bytes, void *payload,
                           size_t payload_bytes, int32_t *status, int token, gi2d_stream_t st) {
    return rans_expand("codec rans expand", kind, n, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask, 0u,
                       tables, tables_bytes, directory, chunk_data, chunk_data_bytes, max_chunk_bytes, payload,
                       payload_bytes, status, token, st);
}

int gi2d_codec_rans_expand_delta(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, int chunk_log2,
                                 unsigned coded_mask, unsigned delta_mask, const void *tables, size_t tables_bytes,
                                 const void *directory, const void *chunk_data, size_t chunk_data_bytes,
                                 size_t max_chunk_bytes, void *payload, size_t payload_bytes, int32_t *status, int token,
                                 gi2d_stream_t st) {
    return rans_expand("codec rans expand delta", kind, n, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2, coded_mask,
                       delta_mask, tables, tables_bytes, directory, chunk_data, chunk_data_bytes, max_chunk_bytes,
                       payload, payload_bytes, status, token, st);
}

size_t gi2d_codec_rans_batch_bytes(int num_streams) { return rans_batch_bytes(num_streams); }

int gi2d_codec_rans_expand_batch(int num_streams, const struct gi2d_codec_rans_stream *streams, void *batch,
                                 size_t batch_bytes, int token, gi2d_stream_t st) {
    const char *what = "codec rans expand batch";
    // ---- everything is checked before anything is launched (and before any device call at all)
    if (num_streams < 1 || num_streams > GI2D_BATCH_MAX)
        return rans_fail(what, "1 .. 64 streams per call", GI2D_ERR_INVALID_ARGUMENT);
    if (!streams || !batch) return rans_fail(what, "null pointer", GI2D_ERR_INVALID_ARGUMENT);
    const RansBatchTable table = carve_rans_batch(batch, num_streams);
    if (batch_bytes < table.bytes || ((uintptr_t)batch & 15))
        return rans_fail(what, "batch table too small (gi2d_codec_rans_batch_bytes) or misaligned", GI2D_ERR_INVALID_ARGUMENT);
    std::vector<RansExpandArgs> args((size_t)num_streams);
    size_t table_b = 0, wave_b = 0;  // the launch's LDS is sized for the most demanding stream of each kind of footprint
    int most_chunks = 0;
    for (int s = 0; s < num_streams; ++s) {
        const gi2d_codec_rans_stream &d = streams[s];
        const std::string who = std::string(what) + ": stream " + std::to_string(s);
        size_t tb, wb;
        const int rc = rans_expand_args(who.c_str(), d.kind, d.num_points, d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits,
                                        d.chunk_log2, d.coded_mask, d.delta_mask, d.tables, d.tables_bytes, d.directory,
                                        d.chunk_data, d.chunk_data_bytes, d.max_chunk_bytes, d.payload, d.payload_bytes,
                                        d.status, token, args[(size_t)s], tb, wb);
        if (rc != GI2D_OK) return rc;
        table_b = tb > table_b ? tb : table_b;
        wave_b = wb > wave_b ? wb : wave_b;
        most_chunks = args[(size_t)s].chunks > most_chunks ? args[(size_t)s].chunks : most_chunks;
    }
    const int waves = rans_expand_waves(table_b, wave_b, most_chunks);
    const size_t lds = table_b + waves * wave_b;
    if (!rans_reserve_lds(what, rans_expand_batched_kernel, lds)) return GI2D_ERR_UNSUPPORTED;
    RansBatchHead head = {};
    long long total = 0;
    for (int s = 0; s < num_streams; ++s) {
        head.wg_start[s] = (int)total;
        total += (args[(size_t)s].chunks + waves - 1) / waves;
    }
    if (total > 0x7fffffffLL) return rans_fail(what, "too many chunks for one launch", GI2D_ERR_INVALID_ARGUMENT);
    head.wg_start[num_streams] = (int)total;
    // ---- the table, stream-ordered, then the one expansion launch
    const hipStream_t q = (hipStream_t)st;
    RansBatchPack pack = {};
    for (int s0 = 0; s0 < num_streams; s0 += GI2D_RANS_BATCH_PACK) {
        const int cnt = num_streams - s0 < GI2D_RANS_BATCH_PACK ? num_streams - s0 : GI2D_RANS_BATCH_PACK;
        for (int i = 0; i < cnt; ++i) pack.args[i] = args[(size_t)(s0 + i)];
        hipLaunchKernelGGL(codec_batch_write_kernel<RansBatchPack>, dim3(1), dim3(256), 0, q, pack,
                           cnt * (int)(sizeof(RansExpandArgs) / sizeof(int)), (int *)(table.args + s0));
    }
    hipLaunchKernelGGL(codec_batch_write_kernel<RansBatchHead>, dim3(1), dim3(256), 0, q, head,
                       (int)(sizeof(RansBatchHead) / sizeof(int)), (int *)table.head);
    hipLaunchKernelGGL(rans_expand_batched_kernel, dim3((unsigned)total), dim3(64 * waves), lds, q,
                       (const RansBatchHead *)table.head, (const RansExpandArgs *)table.args, num_streams);
    return check_launch(what);
}

int gi2d_codec_position_keys(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, const void *payload,
                             size_t payload_bytes, int32_t *keys, gi2d_stream_t st) {
    const char *what = "codec position keys";
    RansLayout L;
    if (!rans_layout(what, kind, xy_bits, p0_bits, p1_bits, color_bits, 8, 0u, L)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 0) return rans_fail(what, "negative size", GI2D_ERR_INVALID_ARGUMENT);
    const long long need = codec_dwords(n, L.rec.record_bits);
    if (payload_bytes < (size_t)need * 4)
        return rans_fail(what, "payload shorter than 4 * ceil(N * R / 32) bytes", GI2D_ERR_INVALID_ARGUMENT);
    if (n == 0) return GI2D_OK;
    if (!payload || !keys || (((uintptr_t)payload | (uintptr_t)keys) & 3))
        return rans_fail(what, "null or misaligned pointer", GI2D_ERR_INVALID_ARGUMENT);
    hipLaunchKernelGGL(codec_position_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)st, n, L,
                       (const uint32_t *)payload, need - 1, keys);
    return check_launch(what);
}

int gi2d_codec_gather(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, const void *payload,
                      size_t payload_bytes, const int32_t *perm, void *out, size_t out_bytes, gi2d_stream_t st) {
    const char *what = "codec gather";
    CodecLayout lay;
    if (!codec_layout(what, kind, xy_bits, p0_bits, p1_bits, color_bits, lay)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 0) return rans_fail(what, "negative size", GI2D_ERR_INVALID_ARGUMENT);
    const long long need = codec_dwords(n, lay.record_bits);
    if (payload_bytes < (size_t)need * 4 || out_bytes < (size_t)need * 4)
        return rans_fail(what, "payload or output shorter than 4 * ceil(N * R / 32) bytes", GI2D_ERR_INVALID_ARGUMENT);
    if (n == 0) return GI2D_OK;
    if (!payload || !perm || !out || payload == out ||
        (((uintptr_t)payload | (uintptr_t)perm | (uintptr_t)out) & 3))
        return rans_fail(what, "null or misaligned pointer, or the output is the input", GI2D_ERR_INVALID_ARGUMENT);
    hipLaunchKernelGGL(codec_gather_kernel, dim3((n + GI2D_CODEC_PACK_BLOCK - 1) / GI2D_CODEC_PACK_BLOCK),
                       dim3(GI2D_CODEC_PACK_BLOCK), 0, (hipStream_t)st, n, lay, (const uint32_t *)payload, need - 1, perm,
                       (uint32_t *)out, need);
    return check_launch(what);
}

}  // extern "C"
