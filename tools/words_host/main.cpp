// The stand-alone host check of csrc/ctcwords.hip (see common.h beside this file and tools/words_host_check.py, which builds and runs it
// with -fsanitize=address,undefined): reads the cases the specification's side exported, runs the ENTRY tatt_ctc_words_read on exactly
// sized heap buffers, one work-group after the other with one thread per lane, and writes every record buffer and lp_out to a file.
//   words_host CASES RESULTS
// CASES, little endian: int32 count, then per case 12 int32 (T, B, C, K, k16, k32, k64, n_codes, n_rows, st_rec, cap, with_lp), the
// float64 word_penalty, int32 codes[n_codes + 1], int32 words[4 K], int32 index[B], float32 logits[T B C] (element (t, b, c) at
// (t B + b) C + c).  RESULTS: per case int32 rc, int32 record[n_rows st_rec] (pre-filled with -77), float64 lp[B T C] (pre-filled 12345).
#include "ctcwords.hip"

thread_local dim3 threadIdx, blockIdx, blockDim;
StandinBlock standin_block;
size_t standin_lds_limit = 64 * 1024;
double wd_lds_base[STANDIN_LDS_BYTES / 8];

void standin_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& body) {
    if (block.x == 0 || block.x % 64 || block.x > 64 * STANDIN_MAX_WAVES || block.y != 1 || block.z != 1 || grid.y != 1 || grid.z != 1 ||
        lds > standin_lds_limit || lds > STANDIN_LDS_BYTES) {
        fprintf(stderr, "standin_launch: no launch of %u threads with %zu bytes of LDS (limit %zu)\n", block.x, lds, standin_lds_limit);
        exit(3);
    }
    for (unsigned bx = 0; bx < grid.x; ++bx) {
        memset(wd_lds_base, 0xa5, sizeof(wd_lds_base));
        standin_block.any = 0;
        pthread_barrier_init(&standin_block.all, nullptr, block.x);
        for (unsigned w = 0; w < block.x / 64; ++w) pthread_barrier_init(&standin_block.wave[w], nullptr, 64);
        std::vector<std::thread> lanes;
        for (unsigned t = 0; t < block.x; ++t)
            lanes.emplace_back([=, &body] {
                threadIdx = dim3(t);
                blockIdx = dim3(bx);
                blockDim = block;
                body();
            });
        for (auto& th : lanes) th.join();
        pthread_barrier_destroy(&standin_block.all);
        for (unsigned w = 0; w < block.x / 64; ++w) pthread_barrier_destroy(&standin_block.wave[w]);
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(wd_lds_base);
        for (size_t i = lds; i < sizeof(wd_lds_base); ++i)
            if (bytes[i] != 0xa5) {
                fprintf(stderr, "work-group %u wrote LDS byte %zu beyond the %zu of its launch\n", bx, i, lds);
                exit(4);
            }
    }
}

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int count = take<int>(in, 1)[0];
    for (int i = 0; i < count; ++i) {
        const std::vector<int> h = take<int>(in, 12);
        const int T = h[0], B = h[1], C = h[2], K = h[3], k16 = h[4], k32 = h[5], k64 = h[6], n_codes = h[7], n_rows = h[8], st_rec = h[9],
                  cap = h[10], with_lp = h[11];
        const double wp = take<double>(in, 1)[0];
        const std::vector<int> codes = take<int>(in, (size_t)n_codes + 1), words = take<int>(in, (size_t)4 * K), index = take<int>(in, B);
        const std::vector<float> logits = take<float>(in, (size_t)T * B * C);
        std::vector<int> record((size_t)n_rows * st_rec, -77);
        std::vector<double> lp((size_t)B * T * C, 12345.0);
        const int rc = tatt_ctc_words_read(logits.data(), (long)B * C, C, 1, T, B, C, codes.data(), n_codes, words.data(), K, k16, k32, k64,
                                           wp, index.data(), record.data(), n_rows, cap, st_rec, with_lp ? lp.data() : nullptr,
                                           (long)T * C, nullptr);
        fwrite(&rc, 4, 1, out);
        fwrite(record.data(), 4, record.size(), out);
        fwrite(lp.data(), 8, lp.size(), out);
        fprintf(stderr, "case %d: T %d, B %d, C %d, K %d: rc %d\n", i, T, B, C, K, rc);
    }
    fclose(in);
    fclose(out);
    return 0;
}
