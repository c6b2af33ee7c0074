// Every tuning knob of libyolo_hip.so, in one place.  Knobs exist for tests, timing ablations and A/B runs; the shipped rules are
// what the library does with all of them at their defaults.
//
// Twelve words are process-wide state: read from the environment at the first use of tuning(), changed afterwards by
// yolo_set_tuning(knob, value) (include/yolo_hip.h), which returns the previous value.
//   knob 0   YOLO_CONV_VARIANT     Tuning::variant          >= 0: tile configuration of the gather kernel by number (choose_igemm in
//                                                           conv_igemm.hip), no other kernel family
//   knob 1   YOLO_CONV_DEBUG       Tuning::conv_debug       kCd* bits
//   knob 2   YOLO_CONV_PP          Tuning::families         kFam* bits
//   knob 3   YOLO_RESUNIT_DEBUG    Tuning::resunit          kRu* bits
//   knob 4   YOLO_MBCONV_DEBUG     Tuning::mbconv           kMb* bits
//   knob 5   YOLO_STEM_DEBUG       Tuning::stem_debug       kStem* bits
//   knob 6   YOLO_STEM_ONE_ROLE    Tuning::stem_one_role    != 0 (the variable: set): stem_kernel (every wave loads and computes) instead
//                                                           of stem2_kernel
//   knob 7   YOLO_MBWIDE_DEBUG     Tuning::mbwide_debug     kMbw* bits
//   knob 8   YOLO_MBWIDE_FORM      Tuning::mbwide_form      1 = 13x13 tiles whenever they fit, 2 = 7x7 tiles always
//   knob 9   YOLO_DWCONV_DEBUG     Tuning::dwconv           kDw* bits
//   knob 10  YOLO_SPP_NO_LINES     Tuning::spp_no_lines     != 0 (the variable: set): the 8-channel SPP form for every shape
//   knob 11  YOLO_RESUNIT_STAGGER  Tuning::resunit_stagger  start offset between the workgroups of a CU (tuning only)
// A bit without a name below is tested nowhere.  Of the named ones, the recipes of tests/_exact_cases.py launch the gather-kernel
// instances behind knob 0 (variants 0, 3, 5, 7, 8, 9, 10, 11) and behind kCdNoLdsEpilogue, kCdNoLoaderWaves, kCd256x256EightWaves,
// kCdMfma32x32, kCdFourWaves, kCdLoadersTwoStages, kCd64x64TwoStages and kCdStreamFirstForm, and compare them bit for bit
// (tests/test_conv_exact_gpu.py); kFamT20Always / kFamT20Never and kFamStreamAlways / kFamStreamNever have their cases there and in
// tests/test_gpu_parity.py.  The form bits of knobs 3 and 4 (kRuGeneric64, kRuT20Always, kRuT20Never, kMbStripForm) select the fused
// kernels of the chained bit-exact cases (tests/_exact_cases.py, tests/test_fused_exact_gpu.py), which ask yolo_resunit_pick /
// yolo_mbconv_pick for the kernel before every launch; kMbStripForm also runs, with the shipped rules of knob 3, on the real
// activation scales in tests/test_gpu_parity.py.  tests/test_pointwise_exact_gpu.py sets kDwOnePixel and kDwFourRows in turn and
// compares the depthwise 3x3 table of tests/_exact_cases.py bit for bit under each.  The ablation bits give wrong results by design
// and have no test.
#pragma once

struct Tuning {
  int variant = -1, conv_debug = 0, families = 0, resunit = 0, mbconv = 0;
  int stem_debug = 0, stem_one_role = 0, mbwide_debug = 0, mbwide_form = 0, dwconv = 0, spp_no_lines = 0, resunit_stagger = 0;
};
Tuning& tuning();   // conv_igemm.hip

// YOLO_CONV_DEBUG / knob 1.  The ablations are for timing only: results are wrong with one of them set.
enum : int {
  kCdNoPixelDma = 1,               // ablation, every conv kernel: no pixel DMA
  kCdNoWeightDma = 2,              // ablation: no weight DMA
  kCdNoMfma = 4,                   // ablation: no MFMA
  kCdNoEpilogue = 8,               // ablation: no epilogue
  kCdNoLdsEpilogue = 16,           // no LDS-staged epilogue (and so only the gather kernel's direct-store instances)
  kCdNoHalo = 32,                  // no halo kernel
  kCdNo128x256 = 128,              // no 128x256 tiles
  kCdNoLoaderWaves = 256,          // no loader waves on the 128x256 tiles of 3x3 layers
  kCd256x256EightWaves = 512,      // 8-wave 256x256 tiles instead of 16-wave
  kCdHalo256Couts = 1024,          // halo kernel: blocks of 256 couts
  kCdMfma32x32 = 2048,             // 32x32x16 MFMA in the gather kernel
  kCdFourWaves = 8192,             // 4-wave 128x128 tiles and 4-wave head tiles
  kCdLoadersTwoStages = 16384,     // two-stage ring for the loader-wave tiles
  kCdTinyGrid64x64 = 32768,        // 64x64 tiles for every tiny-grid 1x1 layer
  kCdHaloMfma32x32 = 65536,        // halo kernel: 32x32x16 MFMA
  kCd64x64TwoStages = 4194304,     // two-stage ring for the 64x64 tiles of the cout-64 layers
  kCdT20NoChunkPairs = 16777216,   // stride-2 20x20-tile kernel: chunk-by-chunk order
  kCdStreamFirstForm = 33554432,   // streaming 1x1: the first (not pipelined) form for the 128-cout layers
  kCdOneTapGeneric = 268435456,    // generic gather path for the 1x1 layers whose cin is not a multiple of 32
};

// YOLO_CONV_PP / knob 2: which kernel FAMILY takes a conv layer
enum : int {
  kFamNoHalo = 8,                  // no halo kernel
  kFamT20Always = 16,              // the 20x20-tile kernels on every layer they can compute
  kFamT20Never = 64,               // ... on none
  kFamStreamNever = 1024,          // the streaming 1x1 kernel on no layer
  kFamStreamAlways = 2048,         // ... on every layer it can compute
};

// YOLO_RESUNIT_DEBUG / knob 3 (fused residual units).  Bit 8 is an ablation in both kernel families, of different phases.
enum : int {
  kRuNoMfmaA = 1,                  // ablation, 16x16-tile kernels: no MFMA of the 1x1
  kRuNoMfmaB = 2,                  // ablation, 16x16-tile kernels: no MFMA of the 3x3
  kRuNoEpilogue = 4,               // ablation, 16x16-tile kernels: no epilogue
  kRuNoPixelDma = 8,               // ablation, 16x16-tile kernels: no pixel DMA of the 1x1
  kRuT20NoEpilogue = 8,            // ablation, 20-pixel-wide tile kernels: no epilogue
  kRuNoMidRows = 16,               // ablation, 16x16-tile kernels: the intermediate is not written to LDS
  kRuGeneric64 = 32,               // generic 16x16-tile kernel for C = 64 instead of the persistent one
  kRuT20Always = 64,               // the 20-pixel-wide tile kernels on every unit they can compute
  kRuT20Never = 128,               // ... on none
  kRuT20OnePerCu = 512,            // 20-pixel-wide tile kernels: one workgroup per CU (diagnosis)
  kRuT20DumpTile0 = 1024,          // ... workgroup 0 dumps its intermediate into y, nobody computes (tools/dbg/ruw_tdump.py)
};

// YOLO_MBCONV_DEBUG / knob 4 (fused MBConv blocks, conv_mbconv.hip)
enum : int {
  kMbFullTile = 1,                 // tile form: never halve the tile
  kMbNoExpand = 2,                 // ablation: no expand stage
  kMbNoDepthwise = 4,              // ablation: no depthwise stage
  kMbNoProject = 8,                // ablation: no projection stage
  kMbNoXLoads = 16,                // ablation: no x loads
  kMbHalfTile = 32,                // tile form: the half tile also below 192 hidden channels
  kMbStripForm = 128,              // the row-strip form where it takes the block (opt-in; tests run both forms)
  kMbFullBarriers = 256,           // tile form: __syncthreads() where the kernel waits for LDS only
};

// YOLO_STEM_DEBUG / knob 5: timing ablations of the fused stem
enum : int {
  kStemNoLoads = 1,                // no input loads
  kStemNoPhaseA = 2,               // no phase A
  kStemNoPhaseB = 4,               // no phase B (stem_kernel only)
  kStemNoStores = 8,               // no stores
  kStemProducersOnly = 64,         // the producer waves alone (stem2_kernel only)
};

// YOLO_MBWIDE_DEBUG / knob 7: timing ablations of the wide MBConv form
enum : int {
  kMbwNoExpand = 2,                // no expand phase
  kMbwNoDepthwise = 4,             // no depthwise phase
  kMbwNoProject = 8,               // no projection phase
  kMbwNoWeightDma = 16,            // no weight DMAs after chunk 0
};

// YOLO_DWCONV_DEBUG / knob 9 (tuning only): both forms give the bits of the shipped 8-row strips
enum : int {
  kDwOnePixel = 1,                 // the one-pixel form
  kDwFourRows = 2,                 // strips of 4 rows instead of 8
};
