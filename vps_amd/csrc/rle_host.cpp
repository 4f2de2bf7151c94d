// Track tubes, host half (vps_amd/tubes.py): the run list of a label map (vps_rle_runs, csrc/rle_ops.hip) -> the compressed COCO
// `counts` string of every wanted key's binary mask. Host-only code: no allocation (the caller passes every buffer), no state, no
// interpreter lock needed, thread-safe.
//   counts  of one key: alternating lengths of zero-runs and one-runs over the positions 0 .. npix-1 in column-major order, starting
//           with a zero-run that may be 0; a trailing zero-run is written only when it is not empty. A key that is absent has the
//           single count npix.
//   string  COCO's rleToString: count i is stored as it is for i <= 2 and as the difference to count i-2 from i = 3 on; the value goes
//           out in groups of 5 bits, low group first, bit 5 = another group follows, each group + 48. The last group is the one after
//           which only the sign is left (the rest is 0 and bit 4 clear, or the rest is -1 and bit 4 set).
// The work is linear in the number of runs: one pass that measures every string, so that the strings can lie one behind the other
// and a short buffer is refused before a byte is stored, and one pass that writes them. tests/rle_restate.py is the NumPy twin.
#include <stdint.h>
#include <string.h>
#include "../../include/vps_hip.h"

#define VPS_EARG(x) (-1000 - (x))

namespace {

constexpr int CHARS_PER_COUNT = 7;              // a difference of two counts below 2^31 has 32 bits and a sign: ceil(33 / 5) groups

struct KeyState {                               // the caller's scratch, four int64 per key
    int64_t pos;                                // positions 0 .. pos-1 are coded
    int64_t n;                                  // counts written
    int64_t c1, c2;                             // counts n-1 and n-2
};

template <bool WRITE>
inline void put_count(KeyState& s, int64_t c, char* dst, int64_t& len) {
    int64_t x = s.n > 2 ? c - s.c2 : c;
    bool more = true;
    while (more) {
        int ch = (int)(x & 0x1f);
        x >>= 5;
        more = (ch & 0x10) ? x != -1 : x != 0;
        if (more) ch |= 0x20;
        if (WRITE) dst[len] = (char)(ch + 48);
        ++len;
    }
    s.c2 = s.c1;
    s.c1 = c;
    ++s.n;
}

inline int find_key(const uint16_t* keys, int nkeys, uint16_t k) {
    int lo = 0, hi = nkeys;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo < nkeys && keys[lo] == k ? lo : -1;
}

// one pass over the runs. WRITE false: length[s] = characters of key s. WRITE true: the characters go to out + offset[s].
template <bool WRITE>
void encode(const uint32_t* run_start, const uint16_t* run_key, int nruns, int64_t npix, const uint16_t* keys, int nkeys, char* out,
            const int64_t* offset, int64_t* length, KeyState* st) {
    for (int s = 0; s < nkeys; ++s) {
        st[s] = KeyState{0, 0, 0, 0};
        length[s] = 0;
    }
    for (int i = 0; i < nruns; ++i) {
        const int s = find_key(keys, nkeys, run_key[i]);
        if (s < 0) continue;
        const int64_t b = run_start[i], e = i + 1 < nruns ? (int64_t)run_start[i + 1] : npix;
        char* dst = WRITE ? out + offset[s] : nullptr;
        put_count<WRITE>(st[s], b - st[s].pos, dst, length[s]);
        put_count<WRITE>(st[s], e - b, dst, length[s]);
        st[s].pos = e;
    }
    for (int s = 0; s < nkeys; ++s)
        if (st[s].pos < npix) put_count<WRITE>(st[s], npix - st[s].pos, WRITE ? out + offset[s] : nullptr, length[s]);
}

}  // namespace

extern "C" int64_t vps_rle_strings_bound(int nruns, int nkeys) {
    if (nruns < 0 || nkeys < 0) return 0;
    // a run of a wanted key adds a zero-run and a one-run, every key at most one more count (the trailing zero-run, or the only one)
    return (int64_t)CHARS_PER_COUNT * (2 * (int64_t)nruns + (int64_t)nkeys);
}

extern "C" int vps_rle_strings(const uint32_t* run_start, const uint16_t* run_key, int nruns, int64_t npix, const uint16_t* keys, int nkeys,
                               char* out, int64_t out_capacity, int64_t* offset, int64_t* length, int64_t* scratch) {
    if (npix <= 0 || npix >= ((int64_t)1 << 31)) return VPS_EARG(4);
    if (nruns < 1 || nruns > npix || !run_start || !run_key) return VPS_EARG(3);
    if (nkeys < 0 || (nkeys > 0 && (!keys || !offset || !length || !scratch))) return VPS_EARG(6);
    if (out_capacity < 0 || (out_capacity > 0 && !out)) return VPS_EARG(8);
    // the list is what vps_rle_runs writes: it starts at 0, positions ascend, neighbours differ in their key
    if (run_start[0] != 0) return VPS_EARG(1);
    for (int i = 1; i < nruns; ++i) {
        if (run_start[i] <= run_start[i - 1] || run_start[i] >= npix) return VPS_EARG(1);
        if (run_key[i] == run_key[i - 1]) return VPS_EARG(2);
    }
    for (int s = 1; s < nkeys; ++s)
        if (keys[s] <= keys[s - 1]) return VPS_EARG(5);
    KeyState* st = reinterpret_cast<KeyState*>(scratch);
    encode<false>(run_start, run_key, nruns, npix, keys, nkeys, nullptr, nullptr, length, st);
    int64_t total = 0;
    for (int s = 0; s < nkeys; ++s) {
        offset[s] = total;
        total += length[s];
    }
    if (total > out_capacity) return VPS_EARG(8);               // offset / length say what is needed; out is untouched
    encode<true>(run_start, run_key, nruns, npix, keys, nkeys, out, offset, length, st);
    return 0;
}
