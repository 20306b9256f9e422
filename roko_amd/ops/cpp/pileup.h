// Sampled-read window feature extraction (the framework's equivalent of the
// reference's generate.cpp:28-160 hot loop, re-architected as a single
// column-store sweep instead of an mpileup multi-iterator + per-column hash
// maps — see SURVEY.md §3.1 for the reference's structure).

#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace rk {

struct FeatureParams {
    int rows = 200;        // sampled read rows per window
    int cols = 90;         // (position, insertion) columns per window
    int stride = 30;       // columns between window starts
    int max_ins = 3;       // insertion slots materialised per position
    uint32_t filter_flag = 0x4 | 0x100 | 0x200 | 0x400 | 0x800;
    uint8_t min_mapq = 10;
    uint64_t seed = 0;     // mixed with (contig, start) by the caller
    // Row sampler. SAMPLER_MT19937 draws rng() % V from one mt19937_64 per
    // region, consumed window after window (the default; its output is
    // frozen). SAMPLER_COUNTER is stateless, so windows can be built in any
    // order (the GPU builder, ops/hip/windows.hip, implements the same rule):
    //   region_key = mix64(seed ^ mix64((tid << 32) ^ start))
    //   draw(w, r) = mix64(region_key ^ mix64((w << 32) | r))
    // row r of window w shows read valid[draw(w, r) % V], w counting every
    // window of the region, skipped empty ones included.
    int sampler = 0;
};

constexpr int SAMPLER_MT19937 = 0;
constexpr int SAMPLER_COUNTER = 1;

// "mt19937" / "counter" -> SAMPLER_*; throws std::invalid_argument otherwise.
int sampler_from_name(const std::string& name);

struct FeatureResult {
    int64_t n_windows = 0;
    std::vector<int32_t> positions;  // n_windows * cols * 2, (ref_pos, ins)
    std::vector<uint8_t> matrices;   // n_windows * rows * cols, base ids 0..11
};

// Build feature windows for pileup columns in [start, end) of `contig`.
// Columns are (position, insertion-slot) pairs; every column covered by the
// filtered pileup enters a sliding queue and windows of `cols` columns are
// emitted every `stride` columns. Rows are reads sampled uniformly WITH
// replacement from the reads overlapping the window (deterministic under
// `seed`). Windows whose column span no read covers are skipped (the
// reference has undefined behaviour there, generate.cpp:123).
FeatureResult extract_features(const std::string& bam_path, const std::string& contig,
                               int64_t start, int64_t end, const FeatureParams& params);

// The filtered reads of a region, still packed as BAM stores them: what the
// device window builder consumes. Same clamping, fetch, filters and read
// order as phase 1 of extract_features; no CIGAR is walked here.
struct RegionReads {
    int64_t start = 0, end = 0;  // clamped region
    int32_t tid = -1;
    uint64_t region_key = 0;     // counter-sampler key of this region
    std::vector<int32_t> ref_start;
    std::vector<int32_t> ref_end;   // exclusive
    std::vector<uint8_t> reverse;
    std::vector<uint32_t> cigar_off{0};  // n + 1, in words
    std::vector<uint32_t> seq_off{0};    // n + 1, in bytes
    std::vector<uint32_t> cigar;         // len << 4 | op
    std::vector<uint8_t> seq4;           // two bases per byte, high nibble first
};

RegionReads region_reads(const std::string& bam_path, const std::string& contig,
                         int64_t start, int64_t end, uint32_t filter_flag,
                         uint8_t min_mapq, uint64_t seed);

}  // namespace rk
