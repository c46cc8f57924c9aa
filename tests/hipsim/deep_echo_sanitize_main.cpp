// Stand-alone host program for a sanitizer run of the Deep Echo engine on the CPU (tests/hipsim/deep_echo_sanitize.sh builds it from the simulator sources with
// -fsanitize=address,undefined and runs it).  It creates a handle from a manifest and a blob, runs ONE call of `batch` rows and writes the int16 output.
//   deep_echo_sanitize <manifest.json> <weights.adew> <input.i16> <batch> <output.i16>
// input: [batch][near end, far end][L] int16, L = the manifest's input_audio_length.
#include "../../include/ade.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s manifest.json weights.adew input.i16 batch output.i16\n", argv[0]); return 2; }
    std::vector<char> manifest = slurp(argv[1]), blob = slurp(argv[2]), in = slurp(argv[3]);
    manifest.push_back('\0');
    const int batch = atoi(argv[4]);
    ade_handle h = nullptr;
    ade_status st = ade_create(manifest.data(), blob.data(), blob.size(), 0, &h);
    if (st != ADE_OK) { fprintf(stderr, "ade_create: %d %s\n", (int)st, ade_last_error(nullptr)); return 1; }
    ade_io_desc io;
    if (ade_get_io(h, &io) != ADE_OK) return 1;
    const size_t want = (size_t)batch * io.in_channels * io.in_len * sizeof(int16_t);
    if (in.size() != want) { fprintf(stderr, "input holds %zu bytes, the call takes %zu\n", in.size(), want); return 2; }
    std::vector<int16_t> out((size_t)batch * io.out_len);
    std::vector<float> f32((size_t)batch * io.out_len);
    st = ade_process(h, reinterpret_cast<const int16_t*>(in.data()), batch, out.data(), f32.data());
    if (st != ADE_OK) { fprintf(stderr, "ade_process: %d %s\n", (int)st, ade_last_error(h)); return 1; }
    std::vector<float> path((size_t)batch * io.frames * 160 * 20);
    size_t written = 0;
    st = ade_debug_tap(h, "path", path.data(), path.size(), &written);
    if (st != ADE_OK || written != path.size()) { fprintf(stderr, "ade_debug_tap(path): %d %s\n", (int)st, ade_last_error(h)); return 1; }
    ade_destroy(h);
    std::ofstream o(argv[5], std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(int16_t)));
    printf("deep_echo_sanitize: %d rows of %d samples, %d frames\n", batch, (int)io.out_len, (int)io.frames);
    return o.good() ? 0 : 1;
}
