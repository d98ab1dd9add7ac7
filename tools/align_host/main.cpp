// The stand-alone host check of csrc/ctcalign.hip (the device stand-in is tools/words_host/common.h, copied beside this file by
// tools/align_host_check.py, which builds and runs the program with -fsanitize=address,undefined): reads the cases the specification's
// side exported, runs the ENTRY tatt_ctc_align on exactly sized heap buffers, one work-group after the other with one thread per lane,
// and writes every record buffer and lp_out to a file.
//   align_host CASES RESULTS
// CASES, little endian: int32 count, then per case 18 int32 (T, B, C, n_rows, rec_stride, rec_at, cap_len, src_rows, src_stride, len_at,
// cls_at, gate_at, src_is_record, with_lp, st_t, st_b, st_c, n_logits), int32 index[B], int32 record[n_rows rec_stride] (its contents
// before the launch), int32 src[src_rows src_stride] (absent where src_is_record), float32 logits[n_logits] (element (t, b, c) at
// t st_t + b st_b + c st_c).  RESULTS: per case int32 rc, int32 record[n_rows rec_stride], float64 lp[B T C] (pre-filled 12345).
#include "ctcalign.hip"

thread_local dim3 threadIdx, blockIdx, blockDim;
StandinBlock standin_block;
size_t standin_lds_limit = 64 * 1024;
double al_lds_base[STANDIN_LDS_BYTES / 8];

void standin_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& body) {
    if (block.x == 0 || block.x % 64 || block.x > 64 * STANDIN_MAX_WAVES || block.y != 1 || block.z != 1 || grid.y != 1 || grid.z != 1 ||
        lds > standin_lds_limit || lds > STANDIN_LDS_BYTES) {
        fprintf(stderr, "standin_launch: no launch of %u threads with %zu bytes of LDS (limit %zu)\n", block.x, lds, standin_lds_limit);
        exit(3);
    }
    for (unsigned bx = 0; bx < grid.x; ++bx) {
        memset(al_lds_base, 0xa5, sizeof(al_lds_base));
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
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(al_lds_base);
        for (size_t i = lds; i < sizeof(al_lds_base); ++i)
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
        const std::vector<int> h = take<int>(in, 18);
        const int T = h[0], B = h[1], C = h[2], n_rows = h[3], rec_stride = h[4], rec_at = h[5], cap_len = h[6], src_rows = h[7],
                  src_stride = h[8], len_at = h[9], cls_at = h[10], gate_at = h[11], src_is_record = h[12], with_lp = h[13];
        const long st_t = h[14], st_b = h[15], st_c = h[16];
        const std::vector<int> index = take<int>(in, B);
        std::vector<long long> record8(((size_t)n_rows * rec_stride + 1) / 2);   // (8-byte aligned, exactly sized for an even stride)
        int* record = reinterpret_cast<int*>(record8.data());
        const std::vector<int> before = take<int>(in, (size_t)n_rows * rec_stride);
        memcpy(record, before.data(), before.size() * 4);
        const std::vector<int> table = take<int>(in, src_is_record ? 0 : (size_t)src_rows * src_stride);
        const std::vector<float> logits = take<float>(in, (size_t)h[17]);
        std::vector<double> lp((size_t)B * T * C, 12345.0);
        const int rc = tatt_ctc_align(logits.data(), st_t, st_b, st_c, T, B, C, index.data(), src_is_record ? record : table.data(), src_rows,
                                      src_stride, len_at, cls_at, gate_at, record, n_rows, rec_stride, rec_at, cap_len,
                                      with_lp ? lp.data() : nullptr, nullptr);
        fwrite(&rc, 4, 1, out);
        fwrite(record, 4, (size_t)n_rows * rec_stride, out);
        fwrite(lp.data(), 8, lp.size(), out);
        fprintf(stderr, "case %d: T %d, B %d, C %d, cap_len %d: rc %d\n", i, T, B, C, cap_len, rc);
    }
    fclose(in);
    fclose(out);
    return 0;
}
