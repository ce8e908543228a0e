// tr_layout_emul.cpp — csrc/tr_layout.h (where the weight-gradient kernels' fill stores a tile in LDS and where their
// transposed reads look for it) compiled for the host, so that tests/test_tr_layout_host.py can check the layout
// without a GPU.  `rowb` selects the instantiation: 128, 256 or 512 bytes per row; anything else returns -1.
#include "../hair-centric-image-retrieval_amd/csrc/tr_layout.h"

extern "C" {

int emul_tr_key(int rowb, int row) {
  return rowb == 128 ? tr_key<128>(row) : rowb == 256 ? tr_key<256>(row) : rowb == 512 ? tr_key<512>(row) : -1;
}

int emul_tr_fill_off(int rowb, int row, int ch16) {
  return rowb == 128   ? tr_fill_off<128>(row, ch16)
         : rowb == 256 ? tr_fill_off<256>(row, ch16)
         : rowb == 512 ? tr_fill_off<512>(row, ch16)
                       : -1;
}

int emul_tr_read_off(int rowb, int row, int c32, int p4) {
  return rowb == 128   ? tr_read_off<128>(row, c32, p4)
         : rowb == 256 ? tr_read_off<256>(row, c32, p4)
         : rowb == 512 ? tr_read_off<512>(row, c32, p4)
                       : -1;
}

int emul_tr_lane_row(int lane, int ks, int hf) { return tr_lane_row(tr_lane(lane), ks, hf); }

int emul_tr_lane_p4(int lane) { return tr_lane(lane).p4; }

}  // extern "C"
