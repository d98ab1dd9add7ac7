// The stand-alone host check of pattern decoding (see tools/words_host/common.h, the thread-per-lane stand-in, and
// tools/pattern_host_check.py, which builds this with beam.cpp under -fsanitize=address,undefined and runs it): reads the cases the
// specification's side exported, runs the ENTRIES tatt_ctc_beam_pattern_read, tatt_ctc_pattern_mass and tatt_ctc_beam_read on exactly
// sized heap buffers, one work-group after the other with one thread per lane, and writes every output buffer to a file.
//   pattern_host CASES RESULTS
// CASES, little endian: int32 count, then per case 12 int32 (T, B, C, beam, nbest, S, n_rows, st_rec, cap, st_mass, plain, 0), uint8
// table[S C], uint8 accept[S], int32 index[B], float32 logits[T B C] (element (t, b, c) at (t B + b) C + c).  plain = 1 also runs
// tatt_ctc_beam_read into a record of its own.
// RESULTS: per case int32 rc of the search, int32 record[n_rows st_rec], int32 rc of the mass, int32 mass[n_rows st_mass], and with
// plain int32 rc, int32 record[n_rows st_rec] (every buffer pre-filled with -77).
#include "ctcpat.hip"

extern "C" int tatt_ctc_beam_pattern_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                                          const unsigned char* table, const unsigned char* accept, int S, const int* index, int* record,
                                          int n_rows, int cap, long st_rec, hipStream_t st);
extern "C" int tatt_ctc_beam_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                                  const int* index, int* record, int n_rows, int cap, long st_rec, hipStream_t st);

thread_local dim3 threadIdx, blockIdx, blockDim;
StandinBlock standin_block;
size_t standin_lds_limit = 64 * 1024;
double cp_lds_base[STANDIN_LDS_BYTES / 8];

void standin_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& body) {
    if (block.x != 64 || block.y != 1 || block.z != 1 || grid.y != 1 || grid.z != 1 || lds > standin_lds_limit || lds > STANDIN_LDS_BYTES) {
        fprintf(stderr, "standin_launch: no launch of %u threads with %zu bytes of LDS (limit %zu)\n", block.x, lds, standin_lds_limit);
        exit(3);
    }
    for (unsigned bx = 0; bx < grid.x; ++bx) {
        memset(cp_lds_base, 0xa5, sizeof(cp_lds_base));
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
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(cp_lds_base);
        for (size_t i = lds; i < sizeof(cp_lds_base); ++i)
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
        const int T = h[0], B = h[1], C = h[2], beam = h[3], nbest = h[4], S = h[5], n_rows = h[6], st_rec = h[7], cap = h[8],
                  st_mass = h[9], plain = h[10];
        const std::vector<unsigned char> table = take<unsigned char>(in, (size_t)(S > 0 ? S : 0) * C);
        const std::vector<unsigned char> accept = take<unsigned char>(in, (size_t)(S > 0 ? S : 0));
        const std::vector<int> index = take<int>(in, B);
        const std::vector<float> logits = take<float>(in, (size_t)T * B * C);
        std::vector<int> record((size_t)n_rows * st_rec, -77), mass((size_t)n_rows * st_mass, -77);
        int rc = tatt_ctc_beam_pattern_read(logits.data(), (long)B * C, C, 1, T, B, C, beam, nbest, table.data(), accept.data(), S,
                                            index.data(), record.data(), n_rows, cap, st_rec, nullptr);
        fwrite(&rc, 4, 1, out);
        fwrite(record.data(), 4, record.size(), out);
        const int rm = tatt_ctc_pattern_mass(logits.data(), (long)B * C, C, 1, T, B, C, table.data(), accept.data(), S, index.data(),
                                             mass.data(), n_rows, st_mass, nullptr);
        fwrite(&rm, 4, 1, out);
        fwrite(mass.data(), 4, mass.size(), out);
        if (plain) {
            std::vector<int> other((size_t)n_rows * st_rec, -77);
            const int rp = tatt_ctc_beam_read(logits.data(), (long)B * C, C, 1, T, B, C, beam, nbest, index.data(), other.data(), n_rows,
                                              cap, st_rec, nullptr);
            fwrite(&rp, 4, 1, out);
            fwrite(other.data(), 4, other.size(), out);
        }
        fprintf(stderr, "case %d: T %d, B %d, C %d, beam %d, S %d: rc %d, %d\n", i, T, B, C, beam, S, rc, rm);
    }
    fclose(in);
    fclose(out);
    return 0;
}
