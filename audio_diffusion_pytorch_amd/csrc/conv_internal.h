// Private to libadp_hip.so: kernel families behind adp_conv1d / adp_conv1d_wgrad (not part of the C-ABI).
#pragma once
#include "adp_rt.h"
#include "adp.h"

// One kernel family of adp_conv1d.  conv1d.hip lists the families in dispatch order (conv_families); the first whose `eligible`
// accepts a descriptor serves its launch AND every query about it, so scratch size, entry counts and launch cannot disagree.
// `eligible` sees the descriptor as the caller has filled it so far (ws, gn_part, gnb_ab, pointer alignment).  A null hook: none / 0.
// (Each file hands out its row through a function: a namespace-scope const object would be emitted into the device code too.)
struct adp_conv_family {
  const char* name;
  bool (*eligible)(const adp_conv_desc& d);
  int (*launch)(const adp_conv_desc& d, void* stream);
  int64_t (*ksplit)(const adp_conv_desc& d);       // potential cross-workgroup K split (sizes d.ws; taken only when d.ws is set)
  int64_t (*gn_entries)(const adp_conv_desc& d);   // gn_part slices per output row quad (store 0, M % 4 == 0)
  int64_t (*gnb_entries)(const adp_conv_desc& d);  // gnb_ab slices per row (store 0, gnb_x 16-byte aligned)
  int64_t (*tile)(const adp_conv_desc& d);         // adp_conv1d_tile code
};
// conv_tile.hip: barrier-free wave-tile kernel (wave-private LDS tile, Winograd F(4,3)) for the HBM-bound 32 -> 32 channel
// kernel-3 ConvBlock convs and their data gradients (depth 1)
const adp_conv_family& adp_family_tile();
// conv_tilek.hip: the same wave tile for the deep layers whose tiles alone cannot fill the chip (>= 512 channels, <= 320 tiles):
// eight waves of a workgroup split the input channels, 16- or 32-row tiles, no cross-workgroup K split / reduce launch
const adp_conv_family& adp_family_tilek();
// conv_mm4.hip: Winograd F(4,3) variant of conv_mm's block for the wide kernel-3 'same' convs without prologue (>= 64 channels,
// >= 200 blocks of 32 rows x 128 positions): MMA waves split the six Winograd planes and the chunk's channels
const adp_conv_family& adp_family_mm4();
// conv_tilek1.hip: tilek's 1x1 sibling (attention projections at batch 1: K split inside the workgroup instead of across workgroups)
const adp_conv_family& adp_family_tilek1();
// conv_mm.hip (+ conv_mm_impl.h, conv_mm_m64/m32.hip): wave-specialised implicit-GEMM conv (stride 1 kernel 1/3,
// kernel = stride 2/4, nearest-upsample loader; channels % 32 == 0)
const adp_conv_family& adp_family_mm();
// conv_direct.hip: VALU direct convolution for the narrow (2-8 channel) ends of the U-Net
const adp_conv_family& adp_family_direct();

// shared by conv_mm.hip and its block-tile translation units
int64_t adp_conv_mm_ksplit(const adp_conv_desc& d);  // cross-workgroup K split the dispatcher picks (1 = none)
bool adp_conv_mm_winograd(const adp_conv_desc& d);   // this conv runs conv_mm's Winograd F(2,3) variant (WN)
int adp_conv_mm_nsp(const adp_conv_desc& d);         // 64-position tiles per block of that variant (1, 2 or 4)
inline bool adp_winograd_enabled() { return adp_knob_on("ADP_CONV_WINO"); }  // (read per call; shared with the weight gradients)

int adp_conv_splitk_reduce(const adp_conv_desc& d, int64_t ks, void* stream);  // sum of d.ws partial tiles + epilogue
int64_t adp_conv_splitk_gn_entries(const adp_conv_desc& d);  // gn_part slices per row the reduce kernel writes
// ADP_GNB_FAMILIES (A/B, bit mask; default all): which kernel families leave the GroupNorm-backward sums -- 1 conv_mm4 12-wave block,
// 2 conv_mm4 light block, 4 conv_tilek, 8 conv_mm, 16 conv_tile32, 32 split-K reduce
inline bool adp_gnb_family_on(int bit) { return (adp_knob("ADP_GNB_FAMILIES", -1) & bit) != 0; }

// The same for adp_conv1d_wgrad (conv1d.hip: wgrad_families).
struct adp_wgrad_family {
  const char* name;
  bool (*eligible)(const adp_wgrad_desc& d);
  int (*launch)(const adp_wgrad_desc& d, void* stream);
  int64_t (*ws_floats)(const adp_wgrad_desc& d);  // scratch a launch needs
  int64_t (*partials)(const adp_wgrad_desc& d);   // partial sums a parked launch leaves in d.ws (null: no parked form, 1)
  int (*launch_n)(const adp_wgrad_desc* ds, int n, void* stream);  // n <= ADP_WGR_BATCH items of one shape in one launch (null: none)
};
constexpr int ADP_WGR_BATCH = 8;
// wgrad_mm.hip: wave-specialised weight gradient of conv_mm's convolutions (channels % 32 == 0)
const adp_wgrad_family& adp_wgrad_family_mm();
// wgrad_direct.hip: VALU streaming weight gradient for the narrow layers (M * R <= 256)
const adp_wgrad_family& adp_wgrad_family_direct();

// second stage of every split weight gradient (wgrad_mm.hip)
int adp_wgrad_reduce(const float* ws, int64_t nsplit, int64_t cnt, int64_t M, float* dw, float* dbias, int accumulate,
                     void* stream);
