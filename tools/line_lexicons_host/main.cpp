// The stand-alone host check of csrc/ctclexp.hip (tools/line_lexicons_host_check.py builds and runs it with -fsanitize=address,undefined
// on the thread-per-lane stand-in of tools/words_host/common.h, which it copies beside this file): reads the cases the specification's
// side exported, runs the ENTRIES tatt_ctc_lexicon_score_pairs and tatt_ctc_lexicon_select_rows on exactly sized heap buffers, one
// work-group after the other with one thread per lane, and writes every score and record buffer to a file.
//   line_lexicons_host CASES RESULTS
// CASES, little endian: int32 count, then per case 12 int32 (T, B, C, U, n_codes, n_tiles, n_pairs, max_count, st_sc, nbest, n_rows,
// st_rec), int32 codes[n_codes + 1], int32 words[4 U], int32 tiles[4 n_tiles], int32 pairs[2 n_pairs], int32 counts[B], int32 index[B],
// float32 logits[T B C] (element (t, b, c) at (t B + b) C + c).  RESULTS: per case int32 rc of the score entry, int32 rc of the select
// entry, float64 scores[B st_sc] (pre-filled with 12345), int32 record[n_rows st_rec] (pre-filled with -77).
#include "ctclexp.hip"

thread_local dim3 threadIdx, blockIdx, blockDim;
StandinBlock standin_block;
size_t standin_lds_limit = 64 * 1024;
double lxp_lds[STANDIN_LDS_BYTES / 8];

void standin_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& body) {
    if (block.x == 0 || block.x % 64 || block.x > 64 * STANDIN_MAX_WAVES || block.y != 1 || block.z != 1 || grid.y != 1 || grid.z != 1 ||
        lds > standin_lds_limit || lds > STANDIN_LDS_BYTES) {
        fprintf(stderr, "standin_launch: no launch of %u threads with %zu bytes of LDS (limit %zu)\n", block.x, lds, standin_lds_limit);
        exit(3);
    }
    for (unsigned bx = 0; bx < grid.x; ++bx) {
        memset(lxp_lds, 0xa5, sizeof(lxp_lds));
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
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(lxp_lds);
        for (size_t i = lds; i < sizeof(lxp_lds); ++i)
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
        const int T = h[0], B = h[1], C = h[2], U = h[3], n_codes = h[4], n_tiles = h[5], n_pairs = h[6], max_count = h[7], st_sc = h[8],
                  nbest = h[9], n_rows = h[10], st_rec = h[11];
        const std::vector<int> codes = take<int>(in, (size_t)n_codes + 1), words = take<int>(in, (size_t)4 * U),
                               tiles = take<int>(in, (size_t)4 * n_tiles), pairs = take<int>(in, (size_t)2 * n_pairs),
                               counts = take<int>(in, B), index = take<int>(in, B);
        const std::vector<float> logits = take<float>(in, (size_t)T * B * C);
        std::vector<double> scores((size_t)B * st_sc, 12345.0);
        std::vector<int> record((size_t)n_rows * st_rec, -77);
        int rc = 0;
        if (n_tiles > 0)
            rc = tatt_ctc_lexicon_score_pairs(logits.data(), (long)B * C, C, 1, T, B, C, codes.data(), n_codes, words.data(), U, tiles.data(),
                                              n_tiles, pairs.data(), n_pairs, counts.data(), max_count, scores.data(), st_sc, nullptr);
        const int rc2 = tatt_ctc_lexicon_select_rows(scores.data(), st_sc, B, counts.data(), nbest, index.data(), record.data(), n_rows,
                                                     st_rec, nullptr);
        fwrite(&rc, 4, 1, out);
        fwrite(&rc2, 4, 1, out);
        fwrite(scores.data(), 8, scores.size(), out);
        fwrite(record.data(), 4, record.size(), out);
        fprintf(stderr, "case %d: T %d, B %d, C %d, U %d, %d tiles, %d pairs: rc %d, %d\n", i, T, B, C, U, n_tiles, n_pairs, rc, rc2);
    }
    fclose(in);
    fclose(out);
    return 0;
}
