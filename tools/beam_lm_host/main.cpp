// The stand-alone host check of csrc/ctcbeam.hip (see common.h beside this file and tools/beam_lm_host_check.py, which builds and runs
// it with -fsanitize=address,undefined): reads the cases the specification's side exported, runs the ENTRIES tatt_ctc_beam_read and
// tatt_ctc_beam_lm_read on exactly sized heap buffers, one work-group after the other with one thread per lane, and writes every record
// buffer to a file.
//   beam_lm_host CASES RESULTS
// CASES, little endian: int32 count, then per case 12 int32 (T, B, C, beam, nbest, order, with_lm, n_rows, st_rec, cap, table entries,
// lm_classes), float64 table[entries], int32 index[B], float32 logits[T B C] (element (t, b, c) at (t B + b) C + c).
// RESULTS: per case int32 rc, int32 record[n_rows st_rec] (pre-filled with -77).
#include "ctcbeam.hip"

thread_local dim3 threadIdx, blockIdx, blockDim;
StandinBlock standin_block;
size_t standin_lds_limit = 64 * 1024;

void standin_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& body) {
    if (block.x != 64 || block.y != 1 || block.z != 1 || grid.y != 1 || grid.z != 1 || lds != 0) {
        fprintf(stderr, "standin_launch: the beam kernel runs one wave per line without dynamic LDS\n");
        exit(3);
    }
    for (unsigned bx = 0; bx < grid.x; ++bx) {
        standin_block.any = 0;
        pthread_barrier_init(&standin_block.all, nullptr, block.x);
        pthread_barrier_init(&standin_block.wave[0], nullptr, 64);
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
        pthread_barrier_destroy(&standin_block.wave[0]);
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
        const int T = h[0], B = h[1], C = h[2], beam = h[3], nbest = h[4], order = h[5], with_lm = h[6], n_rows = h[7], st_rec = h[8],
                  cap = h[9], entries = h[10], lm_classes = h[11];
        const std::vector<double> table = take<double>(in, (size_t)entries);
        const std::vector<int> index = take<int>(in, B);
        const std::vector<float> logits = take<float>(in, (size_t)T * B * C);
        std::vector<int> record((size_t)n_rows * st_rec, -77);
        const int rc = with_lm ? tatt_ctc_beam_lm_read(logits.data(), (long)B * C, C, 1, T, B, C, beam, nbest, table.data(), order,
                                                       lm_classes, index.data(), record.data(), n_rows, cap, st_rec, nullptr)
                               : tatt_ctc_beam_read(logits.data(), (long)B * C, C, 1, T, B, C, beam, nbest, index.data(), record.data(),
                                                    n_rows, cap, st_rec, nullptr);
        fwrite(&rc, 4, 1, out);
        fwrite(record.data(), 4, record.size(), out);
        fprintf(stderr, "case %d: T %d, B %d, C %d, beam %d, order %d, lm %d: rc %d\n", i, T, B, C, beam, order, with_lm, rc);
    }
    fclose(in);
    fclose(out);
    return 0;
}
