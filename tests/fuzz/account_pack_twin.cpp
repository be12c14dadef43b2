// The device reader of a Proof-of-Account job (mina_bridge_amd/csrc/account_pack.cuh), compiled for the HOST: the same text the gfx950 kernels acct_frontend_kernel
// and acct_verdict_kernel are built from, with the stand-in runtime header of this directory (hip_stub) and one "lane" after the other.
// tests/test_account_pack_abi.py builds it with the C++ compiler, feeds it serialized (MinaAccountProof, MinaAccountPubInputs) pairs and compares every output with
// the library's host readers (mina_parse_merkle_path, mina_parse_account_pub_inputs, mina_account_abi_encode) and with the oracle's `to_input` fields: the reader
// logic is checked without a GPU; the GPU tier (tests/test_account_job_gpu.py) then checks the kernels themselves, Poseidon stages included.
//
//   account_pack_twin IN OUT
//   IN:  u64 blob_len; blob; u64 n; n u64 proof_off; n u64 proof_len; n u64 pub_off; n u64 pub_len; n*32 roots (what the fold would have produced)
//   OUT: 4n records; 4n u32 field counts; 4n u32 salt indices; n*64*32 siblings; n*64 dirs; n u32 depths; n*32 ledger hashes; n u32 zkApp marks; n u32 zk_index;
//        u32 zk_count; n u32 bits; n u32 passed; n u32 ran                      (memory the reader does not write is zero)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

static inline unsigned long long __brevll(unsigned long long x) { unsigned long long r = 0; for (int i = 0; i < 64; ++i) r |= ((x >> i) & 1ull) << (63 - i); return r; }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }

#include "../../mina_bridge_amd/csrc/account_pack.cuh"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE *f, const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: account_pack_twin IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t blob_len = 0, n = 0;
    if (!rd(in, &blob_len, 1)) return 2;
    std::vector<uint8_t> blob(blob_len + 1);
    if (!rd(in, blob.data(), blob_len) || !rd(in, &n, 1)) return 2;
    std::vector<uint64_t> po(n), pl(n), qo(n), ql(n);
    std::vector<uint4> roots(2 * n), rec(mb::AS_STAGES * n * mb::ACCT_REC16, uint4{0, 0, 0, 0}), sib(n * mb::ACCT_MAX_DEPTH * 2, uint4{0, 0, 0, 0}), ledger(2 * n, uint4{9, 9, 9, 9});
    if (!rd(in, po.data(), n) || !rd(in, pl.data(), n) || !rd(in, qo.data(), n) || !rd(in, ql.data(), n) || !rd(in, roots.data(), 2 * n)) return 2;
    std::vector<uint32_t> nf(mb::AS_STAGES * n, 0), salt(mb::AS_STAGES * n, 0), depth(n, 99), marks(n, 9), zk_index(n, 0), bits(n, 0), passed(n, 0), ran(n, 0);
    std::vector<uint8_t> dirs(n * mb::ACCT_MAX_DEPTH, 0);
    uint32_t zk_count = 0;
    for (uint64_t i = 0; i < n; ++i)
        mb::acct_frontend_entry((uint32_t)i, (uint32_t)n, blob.data(), blob_len, po.data(), pl.data(), qo.data(), ql.data(), rec.data(), nf.data(), salt.data(), sib.data(), dirs.data(),
                                depth.data(), ledger.data(), marks.data(), zk_index.data(), &zk_count, bits.data());
    for (uint64_t i = 0; i < n; ++i) mb::acct_verdict_entry((uint32_t)i, bits.data(), roots.data(), ledger.data(), passed.data(), ran.data());
    wr(out, rec.data(), rec.size()); wr(out, nf.data(), nf.size()); wr(out, salt.data(), salt.size()); wr(out, sib.data(), sib.size()); wr(out, dirs.data(), dirs.size());
    wr(out, depth.data(), n); wr(out, ledger.data(), 2 * n); wr(out, marks.data(), n); wr(out, zk_index.data(), n); wr(out, &zk_count, 1); wr(out, bits.data(), n);
    wr(out, passed.data(), n); wr(out, ran.data(), n);
    fclose(in); return fclose(out) == 0 ? 0 : 2;
}
