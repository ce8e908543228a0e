// jpeg_stream_check.cpp — TEST INFRASTRUCTURE.  A stand-alone program (its own main) that takes every file of a
// directory through the JPEG path's host code and host-compiled device code — jpeg_host::parse, jpeg_host::stage and the
// emulated decode of tests/jpeg_emul.cpp, i.e. jpeg_core.h / jpeg_stage.h exactly as the emulator includes them — and
// then does the same with the file cut short at every `stride`-th byte.  A whole file must decode (status 0); a
// truncation must be parsed or rejected; neither may touch memory outside its buffers.  Built by
// tests/test_jpeg_host.py with g++ -fsanitize=address,undefined -fno-sanitize-recover=all and run as a subprocess:
// every input sits in a heap block of exactly its size, so a read past the end of the file is reported.
// Usage: jpeg_stream_check DIR [stride = 97]
#include <dirent.h>
#include <stdio.h>

#include <algorithm>
#include <string>

#include "jpeg_emul.cpp"

namespace {

bool read_file(const std::string& path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t n;
  out.clear();
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

// parse + stage + decode `n` bytes held in a heap block of exactly n bytes; returns the decode's status
int run(const uint8_t* data, size_t n, int32_t threads, bool whole_image) {
  uint8_t* exact = static_cast<uint8_t*>(malloc(n ? n : 1));
  memcpy(exact, data, n);
  int rc;
  {
    hcir_jpeg_header h;
    jpeg_host::Scan sc;
    rc = jpeg_host::parse(exact, n, &h, &sc);
    if (rc == HCIR_OK) {
      std::vector<uint8_t> blob(jpeg_host::stage_bound(h, sc));
      size_t used = 0;
      rc = jpeg_host::stage(&h, sc, blob.data(), &used);
      if (rc == HCIR_OK && used > blob.size()) {
        fprintf(stderr, "stage used %zu of %zu bytes\n", used, blob.size());
        abort();
      }
      if (rc == HCIR_OK) {
        const int32_t wh = whole_image ? h.height : 24, ww = whole_image ? h.width : 40;
        std::vector<uint8_t> out((size_t)wh * ww * 3);
        int32_t stats[8] = {0};
        rc = emul_decode_window(exact, n, wh, ww, threads, out.data(), stats);
      }
    }
  }
  free(exact);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s DIR [stride]\n", argv[0]);
    return 2;
  }
  const size_t stride = argc > 2 ? (size_t)atoi(argv[2]) : 97;
  if (stride == 0) return 2;
  std::vector<std::string> names;
  DIR* d = opendir(argv[1]);
  if (!d) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  while (dirent* e = readdir(d))
    if (e->d_name[0] != '.') names.push_back(e->d_name);
  closedir(d);
  std::sort(names.begin(), names.end());
  size_t nfiles = 0, ntrunc = 0, ntrunc_ok = 0, nbad = 0;
  for (const std::string& name : names) {
    std::vector<uint8_t> file;
    if (!read_file(std::string(argv[1]) + "/" + name, file)) {
      fprintf(stderr, "cannot read %s\n", name.c_str());
      return 2;
    }
    ++nfiles;
    // a name that starts with "reject_" must be refused by the stager, every other file must decode
    const bool reject = name.compare(0, 7, "reject_") == 0;
    const int32_t configs[4] = {1024, 512, 96, -1024};
    for (int32_t t : configs) {
      const int rc = run(file.data(), file.size(), t, true);
      if ((rc == HCIR_OK) == reject) {
        fprintf(stderr, "%s: status %d at %d threads\n", name.c_str(), rc, t);
        ++nbad;
      }
    }
    for (size_t n = 0; n < file.size(); n += stride) {
      ++ntrunc;
      ntrunc_ok += run(file.data(), n, 96, (n / stride) % 2 == 0) == HCIR_OK;
    }
  }
  printf("files %zu truncations %zu decoded_truncations %zu failures %zu\n", nfiles, ntrunc, ntrunc_ok, nbad);
  return nbad ? 1 : 0;
}
