// The device front end of a Proof-of-State job (mina_bridge_amd/csrc/state_pack.cuh), compiled for the HOST: the same text the gfx950 kernels are built from,
// with the stand-in runtime header of this directory (hip_stub) and one "lane" after the other.  tests/test_state_pack_abi.py builds it with the C++ compiler,
// feeds it serialized protocol states and compares every output byte with the library's host reader (mina_protocol_state_pack, the consensus entry points):
// the reader logic is checked without a GPU; the GPU tier (tests/test_state_pack_gpu.py) then checks the kernels themselves.
//
//   state_pack_twin IN OUT
//   IN:  u32 mode; u64 blob_len; blob;
//        mode 0 (pstate_pack_kernel, info for every state):   u64 n; n u64 off; n u32 len
//        mode 1 (the four kernels of mina_state_frontend_dev): u64 batch; batch u64 begin; batch u64 end; batch*17*32 expected; batch*16*32 ledger; batch u8 and
//   OUT: mode 0: per state  u8 status, u32 n_body_fields, the record, the info struct
//        mode 1: batch*17 records; batch*17 u32 field counts; batch u8 precheck; batch u32 masks
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

static inline unsigned __brev(unsigned x) { unsigned r = 0; for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i); return r; }
static inline unsigned long long __brevll(unsigned long long x) { unsigned long long r = 0; for (int i = 0; i < 64; ++i) r |= ((x >> i) & 1ull) << (63 - i); return r; }

#include "../../mina_bridge_amd/csrc/state_pack.cuh"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE *f, const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: state_pack_twin IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t mode = 0; uint64_t blob_len = 0, n = 0;
    if (!rd(in, &mode, 1) || !rd(in, &blob_len, 1)) return 2;
    std::vector<uint8_t> blob(blob_len + 1);
    if (!rd(in, blob.data(), blob_len) || !rd(in, &n, 1)) return 2;
    constexpr size_t REC16 = mb::PSTATE_REC_BYTES / 16;
    if (mode == 0) {
        std::vector<uint64_t> off(n); std::vector<uint32_t> len(n), nf(n), info(n * mb::PI_WORDS, 0xa5a5a5a5u); std::vector<uint4> rec(n * REC16, uint4{7, 7, 7, 7}); std::vector<uint8_t> status(n, 9);
        if (!rd(in, off.data(), n) || !rd(in, len.data(), n)) return 2;
        for (uint64_t i = 0; i < n; ++i) mb::pstate_pack_entry((uint32_t)i, blob.data(), blob_len, off.data(), len.data(), rec.data(), nf.data(), info.data(), 0, status.data());
        for (uint64_t i = 0; i < n; ++i) { wr(out, &status[i], 1); wr(out, &nf[i], 1); wr(out, &rec[i * REC16], REC16); wr(out, &info[i * mb::PI_WORDS], mb::PI_WORDS); }
    } else {
        const uint64_t ns = n * MINA_STATES_PER_PROOF;
        std::vector<uint64_t> begin(n), end(n), off(ns), ledger(n * 16 * 4); std::vector<uint32_t> len(ns), nf(ns, 77), info(2 * n * mb::PI_WORDS), masks(n);
        std::vector<uint8_t> expected(ns * 32), band(n), status(ns), fmt(n), pre(n); std::vector<uint4> rec(ns * REC16, uint4{7, 7, 7, 7});
        if (!rd(in, begin.data(), n) || !rd(in, end.data(), n) || !rd(in, expected.data(), ns * 32) || !rd(in, ledger.data(), n * 64) || !rd(in, band.data(), n)) return 2;
        for (uint64_t b = 0; b < n; ++b) mb::pstate_split_entry((uint32_t)b, blob.data(), blob_len, begin.data(), end.data(), off.data(), len.data(), fmt.data());
        for (uint64_t i = 0; i < ns; ++i) mb::pstate_pack_entry((uint32_t)i, blob.data(), blob_len, off.data(), len.data(), rec.data(), nf.data(), info.data(), 1, status.data());
        for (uint64_t b = 0; b < n; ++b) mb::pstate_precheck_entry((uint32_t)b, rec.data(), status.data(), info.data(), expected.data(), ledger.data(), band.data(), fmt.data(), pre.data(), masks.data());
        for (uint64_t b = 0; b < n; ++b) if (!fmt[b]) {          // pstate_clear_kernel
            for (size_t t = 0; t < MINA_STATES_PER_PROOF * REC16; ++t) rec[b * MINA_STATES_PER_PROOF * REC16 + t] = uint4{0, 0, 0, 0};
            for (size_t t = 0; t < MINA_STATES_PER_PROOF; ++t) nf[b * MINA_STATES_PER_PROOF + t] = 0;
        }
        wr(out, rec.data(), rec.size()); wr(out, nf.data(), ns); wr(out, pre.data(), n); wr(out, masks.data(), n);
    }
    fclose(in); return fclose(out) == 0 ? 0 : 2;
}
