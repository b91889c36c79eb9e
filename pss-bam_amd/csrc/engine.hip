// pss-bam_amd/csrc/engine.hip -- the C ABI declared in include/pssbam_hip.h.
//
// Host side of the MI355X tally engine: device-resident genome, BAM refID -> contig map
// with find_seq semantics, double-buffered H2D staging of record blocks, kernel choice
// and launch geometry, u64 counter block.  Written for gfx950 only; there is no CPU path.
#include "../../include/pssbam_hip.h"
#include "../../include/fasta-genome-io.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "tally_kernels.h"
#include "select_kernels.h"
#include "end_mask_kernels.h"
#include "dedup_kernels.h"
#include "coverage_kernels.h"
#include "allele_kernels.h"
#include "deflate_kernels.h"

using namespace pssbam;

// --------------------------------------------------------------------------------------
// errors
// --------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static double feed_now() {   // host seconds, for the PSSBAM_STATS lines
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(PSSBAM_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

extern "C" const char *pssbam_last_error(void) { return g_err; }

static bool device_is_gfx950(int dev) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return false;
    return strncmp(pr.gcnArchName, "gfx950", 6) == 0;
}

extern "C" int pssbam_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < n; d++) ok += device_is_gfx950(d) ? 1 : 0;
    return ok;
}

extern "C" int pssbam_warmup(int device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(nullptr));  // forces the context
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// engine
// --------------------------------------------------------------------------------------
struct Slot {  // one in-flight host-submitted block
    uint8_t *d_recs = nullptr;
    size_t recs_cap = 0;
    uint32_t *d_offs = nullptr;
    size_t offs_cap = 0;  // entries
    hipEvent_t copy_begin = nullptr, copied = nullptr, consumed = nullptr;
    bool busy = false;
    bool timed = false;       // copy_begin/copied hold an unread H2D duration
    uint64_t ticket = 0;      // the submit that last used the slot
};

// per super-batch: the output of ONE round of the inflate kernel's 65 536 lanes (a block per lane: 4.28 GB at htslib's
// 65 280-byte blocks) and room for its compressed bytes.  Super-batches live in a ring of slots that grows while the tally
// launches wait for the genome (pssbam_engine_feed_open) and is three deep otherwise.
static constexpr uint64_t FEED_OUT_TARGET = 4400ull << 20, FEED_COMP_CAP = 2ull << 30, FEED_OUT_SLACK = 160ull << 20,
                          FEED_OVERSHOOT = 64ull << 20,   // a submit may run this far past the target before the super-batch is cut
                          FEED_GAP = 16ull << 20,   // room in front of a super-batch's data for the record the previous one ended in
                          FEED_SUB_MAX = 3584ull << 20;   // record bytes per tally launch: below 4 GiB
static constexpr int FEED_SLOTS_READY = 3, FEED_SLOTS_MAX = 40;

struct FeedAcc {  // one super-batch of compressed blocks: assembled chunk by chunk, then inflated in ONE launch
    uint8_t *d_comp = nullptr;      // compressed bytes of the chunks, back to back (each 16-byte aligned)
    size_t comp_cap = 0;
    uint64_t comp_used = 0;
    std::vector<pssbam_bgzf_block> blocks;   // in_off into d_comp, out_off into d_out (contiguous from FEED_GAP on)
    std::vector<uint32_t> sub_first;         // first block of every tally sub-batch (< 4 GiB of records each)
    uint64_t out_used = 0, sub_bytes = 0;
    void *d_blocks = nullptr;                // pssbam::BgzfBlock[]
    pssbam_bgzf_block *h_blocks = nullptr;   // page-locked copy of `blocks` for the upload (a pageable source makes hipMemcpyAsync wait for the stream)
    size_t h_blocks_cap = 0;
    // per block: chain pieces (first record start, records, end, last record start), suffix minimum, counts, bases
    uint64_t *d_a = nullptr, *d_e = nullptr, *d_last = nullptr, *d_nexta = nullptr;
    uint32_t *d_n = nullptr, *d_counts = nullptr, *d_base = nullptr;
    size_t blocks_cap = 0;
    uint8_t *d_out = nullptr;                // [0, FEED_GAP): the partial record carried over from the previous super-batch
    size_t out_cap = 0;
    uint32_t *d_offs = nullptr;
    size_t offs_cap = 0;
    uint32_t *d_nrecs = nullptr;
    size_t nrecs_cap = 0;
    uint64_t *d_chain = nullptr;             // [0] where this super-batch's chain starts, [1] where its tail starts, [2] links broken, [3] links repaired
    hipEvent_t consumed = nullptr, copies_done = nullptr, copies_done2 = nullptr, inflated = nullptr, inflate_done = nullptr;
    bool busy = false;                       // flushed; its buffers are in use until `consumed`
    bool held = false;                       // ... and its tally launches still wait for the genome (no `consumed` yet)
    uint64_t flush_seq = 0;                  // order of the flushes (the oldest busy slot frees first)
};

struct DeferredTally {   // a tally launch that waits for set_genome + set_references (pssbam_engine_feed_open)
    int slot;
    uint64_t sub_base, sub_len, offs_at;
    uint32_t n_bound, k;
    uint64_t sample_off;
    bool last_of_slot;
};

// Host ranges page-locked for genome uploads, shared by the engines of a process (one engine per GPU uploads the same
// contigs): registered once, released when the last upload that uses them has completed.
namespace {
struct PinEntry { size_t len; int refs; };
std::map<const void *, PinEntry> g_pins;
std::mutex g_pins_mu;
bool pin_acquire(const void *p, size_t len) {
    std::lock_guard<std::mutex> lk(g_pins_mu);
    auto it = g_pins.find(p);
    if (it != g_pins.end()) { it->second.refs++; return true; }
    if (hipHostRegister((void *)p, len, hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); return false; }
    g_pins[p] = PinEntry{len, 1};
    return true;
}
void pin_release(const void *p) {
    std::lock_guard<std::mutex> lk(g_pins_mu);
    auto it = g_pins.find(p);
    if (it == g_pins.end()) return;
    if (--it->second.refs == 0) { (void)hipHostUnregister((void *)p); g_pins.erase(it); }
}
}  // namespace

// One of the record sink's two output buffers (pssbam_engine_set_record_sink): the kept records of one tally launch on the
// device, their {bytes, records} totals (with the block sink {raw bytes, records, compressed bytes, blocks}), and the page-locked host memory both are copied to.  free -> the selection is
// queued and the totals are on their way (SEL_TOTALS) -> the totals are known and the data is on its way (SEL_DATA) ->
// delivered, free again.
enum SelectState { SEL_FREE = 0, SEL_TOTALS, SEL_DATA };
struct SelectBuf {
    uint8_t *d_out = nullptr;
    size_t out_cap = 0;
    unsigned long long *d_totals = nullptr, *h_totals = nullptr;
    uint8_t *h_data = nullptr;
    size_t h_cap = 0;
    hipEvent_t totals_ev = nullptr, data_ev = nullptr;
    SelectState state = SEL_FREE;
    bool deflated = false;   // the block sink's: d_out holds totals[3] BGZF blocks in totals[2] bytes
};

struct KernelPrep { uint32_t lds = 0; int occ = 0; };   // tiled_grid's memo of one kernel: dynamic-LDS limit set, occupancy at it

struct pssbam_engine {
    pssbam_config cfg{};
    std::string up_ctx, down_ctx, rg;
    bool has_rg = false;
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr, copy_stream = nullptr, copy_stream2 = nullptr;
    hipStream_t inflate_stream[2] = {nullptr, nullptr};   // PSSBAM_FEED_INFLATE_STREAMS=2: the feed's inflate launches take turns on these (bgzf_api.h feed_flush; off by default)
    hipEvent_t feed_base_ev = nullptr;                    // time zero of the feed's kernel intervals (feed_status: their union)
    hipStream_t genome_stream = nullptr;   // genome upload + encode + pack: beside whatever the engine's stream runs
    // A HIP stream costs 20-30 ms to create (a hardware queue each): only the engine's own is made before create returns;
    // the copy streams and the genome's are made by a helper thread while the first blocks go out -- those are copied on
    // the engine's stream, in front of the kernel that reads them anyway -- and adopted when they are there (late_streams()).
    std::thread late_thread;
    std::atomic<int> late_ready{0};
    std::mutex late_mu;
    hipStream_t late_copy1 = nullptr, late_copy2 = nullptr, late_genome = nullptr;
    bool late_adopted = false;
    hipEvent_t genome_ready = nullptr;
    bool genome_wait_pending = false;      // the next tally launch makes the engine's stream wait for genome_ready
    std::vector<const void *> genome_pins; // host contigs page-locked for an upload still in flight
    std::vector<void *> retired;           // device buffers replaced while kernels might still read them: freed at destroy
    hipEvent_t copied2 = nullptr;   // second half of a split H2D copy
    bool own_stream = false;

    // genome
    uint8_t *d_genome = nullptr;
    uint32_t *d_genome4 = nullptr;  // 4-bit image for the tiled kernel's window gathers
    uint32_t acgt_ctx = 0;
    uint64_t genome_bytes = 0;
    std::vector<uint64_t> contig_start;  // per sorted contig
    std::vector<uint32_t> contig_len;
    std::vector<std::string> contig_ids;  // sorted by strcmp, like Genome.seqs
    int32_t star_contig = -1;
    // references
    uint4 *d_ref_info = nullptr;  // n_ref + 1 entries (last = RNAME "*")
    uint4 *h_ref_info = nullptr;  // the same in page-locked host memory: a kernel copies it over (below)
    size_t h_ref_cap = 0;
    int32_t n_ref = 0;
    bool have_refs = false;
    // -R
    uint8_t *d_rg = nullptr;
    // -G / -S / -C: n_planes [fwd | rev] planes of the counter block behind the stats (set_planes); plane 1 + g holds
    // read group g (pssbam_engine_set_read_groups), length bin g (pssbam_engine_set_length_bins), replicate g (pssbam_engine_set_replicates) or contig set g
    // (pssbam_engine_set_contig_sets)
    PlaneSel planes = PLANES_NONE;
    uint32_t n_planes = 0, off_groups = 0, plane_words = 0;
    uint64_t kplane_words = 0;   // a k-mer engine's plane: one [k5 | k3] pair, 2 * 4^k words (64-bit: 2^31 at k = 15)
    uint8_t *d_grp_ids = nullptr;   // -G: the ID table
    uint32_t *d_grp_offs = nullptr, *d_grp_hash = nullptr;
    uint32_t grp_hash_mask = 0;
    std::vector<uint32_t> len_edges;   // -S
    std::unordered_map<std::string, uint32_t> ctg_plane;   // -C: contig name -> 1 + set, packed into ref_info[].w
    std::vector<std::string> ref_names;   // the names of the last set_references (-C set after it packs them again)
    // -A (pssbam_engine_set_per_contig): planes == PLANES_EACH, n_planes = n_ref + 1 once the reference count is known (plane k
    // = refID k at off_groups + k * plane_words, the last one refID -1), and behind the planes one touched word per plane
    bool per_contig = false;
    uint64_t off_touched = 0;
    int env_contig_slots = 0;   // PSSBAM_CONTIG_SLOTS: LDS planes a workgroup of the -A kernel holds (tests: down to 1)
    bool contig_evict = true;   // PSSBAM_CONTIG_EVICT=0: the -A kernel empties its slots at a miss only (A/B runs)
    bool tallied = false;   // a tally launch since create / reset
    uint32_t min_bq = 0;    // -Q: read bases with a QUAL byte below this are left out of the tables (pssbam_engine_set_min_base_quality)
    // -H (pssbam_engine_set_length_histogram): hf | hr, hist_max + 2 words each, at off_groups = the end of the block as it is without them
    uint32_t hist_max = 0;
    // -X (pssbam_engine_set_site_context): fwd_in | rev_in, rows * 16 words each, at off_groups = the end of the block as it is without them
    uint32_t site_mode = 0;
    // -E (pssbam_engine_set_end_condition): fwd_c | rev_c | reads[4], rows * 16 words per table, at off_groups = the end of the block as it is without them
    uint32_t end_depth = 0, end_cell5 = 0, end_cell3 = 0;
    // -n / -N / -V (pssbam_engine_set_mismatches): mf | mr, mism_hist + 2 words each, at off_groups = the end of the block as it is without
    // them (mism_hist = 0: no words); mism_max = -1: no filter
    uint32_t mism_hist = 0;
    int32_t mism_max = -1;
    bool mism_tv = false;
    // -W (pssbam_engine_set_interior): table[16] | reads, 17 words at off_groups = the end of the block as it is without them;
    // interior_margin = -1: off, no words
    int32_t interior_margin = -1;
    // -P (pssbam_engine_set_composition): c5 | c3, 2 * width * 5 words each at off_groups = the end of the block as it is
    // without them; composition = 0: off, no words
    uint32_t composition = 0;
    // -y / -Y (pssbam_engine_set_read_score): the weights [4][score_nd][score_nq] in device memory (d_score_w = NULL: off); the
    // filter S >= score_min when score_filter; sf | sr, 2 * score_half words each at off_groups = the end of the block as it is
    // without them (score_half = 0: no words)
    int16_t *d_score_w = nullptr;
    uint32_t score_nd = 0, score_nq = 0, score_half = 0, score_shift = 0;
    int32_t score_min = 0;
    bool score_filter = false;
    // the record sink (pssbam_engine_set_record_sink, select_kernels.h).  Without one nothing below is allocated and nothing
    // more is launched.  sel_queue: the buffers in flight, oldest first (the order of delivery).
    pssbam_record_sink sink = nullptr;
    void *sink_ctx = nullptr;
    bool sink_failed = false;          // the sink returned non-zero and no engine call has reported it yet (select_report)
    // the block sink (pssbam_engine_set_block_sink, deflate_kernels.h): the same selection, deflated into BGZF blocks behind
    // the gather.  One or the other is set.  d_comp: a 64 KiB slot per block of the chunk being deflated, shared by both
    // selection buffers (stream order keeps the chunks apart); the packed blocks go back into the chunk's own d_out.
    pssbam_block_sink block_sink = nullptr;
    void *block_ctx = nullptr;
    bool block_sink_failed = false;    // which of the two sink_failed speaks of
    uint8_t *d_comp = nullptr;
    size_t comp_cap = 0;               // in blocks
    uint32_t *d_comp_len = nullptr;
    unsigned long long *d_comp_off = nullptr;
    SelectBuf sel[2];
    int sel_next = 0;
    std::vector<int> sel_queue;
    uint32_t *d_sel_len = nullptr;     // len[] / dst[] of the launch being selected (stream order keeps the launches apart)
    size_t sel_len_cap = 0;
    uint2 *d_sel_sums = nullptr;
    size_t sel_sums_cap = 0;
    hipStream_t sel_stream = nullptr;  // the D2H copies of the kept records, beside the next block's kernels
    uint64_t sel_launches = 0;         // (not part of kernel_launches: that count is the tally's)
    // the end mask (pssbam_engine_set_end_mask, end_mask_kernels.h): one kernel between the gather and the deflate, nothing of its own
    uint32_t end_mask_mode = PSSBAM_END_MASK_OFF, end_mask_n5 = 0, end_mask_n3 = 0;
    // duplicate flagging (pssbam_engine_set_duplicates, dedup_kernels.h).  Off: nothing below is allocated and nothing more is launched.
    // The table holds dedup_cap slots (a power of two, 0: not allocated yet); d_dedup_slot is slot_of[] of the block being flagged
    // (stream order keeps the blocks apart); d_dedup_state the device's {occupied slots | DEDUP_FULL}, read back through
    // h_dedup_state behind a block's resolve kernel and an event that is polled, never waited on: dedup_known is the last value
    // that arrived and dedup_known_at the records submitted up to that reading (the host's bound), dedup_submitted all of them.
    bool dedup = false;
    uint32_t dedup_initial = 0;        // the first table's slots as the caller asked (0: DEDUP_DEFAULT_SLOTS)
    DedupSlot *d_dedup = nullptr;
    uint64_t dedup_cap = 0;
    uint32_t *d_dedup_slot = nullptr;
    size_t dedup_slot_cap = 0;
    unsigned long long *d_dedup_state = nullptr, *h_dedup_state = nullptr;
    hipEvent_t dedup_ev = nullptr;
    bool dedup_reading = false;        // a copy of the state word is on its way
    uint64_t dedup_known = 0, dedup_known_at = 0, dedup_reading_at = 0, dedup_submitted = 0;
    uint32_t dedup_seq = 0;            // blocks flagged since create / reset: the high word of a record's ordinal
    uint64_t dedup_launches = 0;       // (not part of kernel_launches: that count is the tally's)
    std::vector<std::pair<void *, hipEvent_t>> dedup_old;   // tables replaced by a larger one: freed once the stream has passed the rehash
    // depth of coverage (pssbam_engine_set_coverage, coverage_kernels.h).  Off: nothing below is allocated and nothing more is launched.
    // d_cov holds the differences, cov_len entries (the stored genome length rounded up to whole tiles; 0: no genome yet -- it is
    // allocated when the genome's size is known); the rest are finish's buffers, kept between calls: per-tile sums and run counts,
    // the totals {histogram, runs, 3 words per listed contig}, and the listed contigs sorted by their place in the genome.
    bool coverage = false;
    uint64_t cov_hint = 0;             // positions_hint of the caller (what the array is expected to take, for the feed's memory budget)
    uint32_t *d_cov = nullptr;
    uint64_t cov_len = 0;
    unsigned long long *d_cov_sums = nullptr, *d_cov_runcnt = nullptr, *d_cov_out = nullptr;
    size_t cov_sums_cap = 0, cov_out_cap = 0;
    uint4 *d_cov_contigs = nullptr;
    size_t cov_contigs_cap = 0;
    std::vector<uint4> cov_contigs;    // the contigs of the reference list, each once, sorted by lo: {lo low, lo high, length, first refID}
    bool cov_contigs_sent = false;
    // what the last finish computed, while nothing has been added since: the totals on the host, the tiles' bases in d_cov_sums,
    // and the tiles' run counts in d_cov_runcnt (cov_runs_scanned: already turned into their exclusive scan)
    bool cov_totals_valid = false, cov_runs_scanned = false;
    std::vector<unsigned long long> cov_out_host;
    uint32_t *d_cov_runs = nullptr;    // finish_coverage_runs' [slot | start | end | depth], cov_runs_cap words each
    uint64_t cov_runs_cap = 0;
    bool gapped = false;   // -I (pssbam_engine_set_gapped_reads): clipped and gapped reads are tallied by their anchored ends; no counter words
    int env_hist_lds_bins = -1;   // PSSBAM_HIST_LDS_BINS: at most this many bins of each array in LDS (tests: the global-atomic path with short reads)
    // -T (pssbam_engine_set_regions): contig name -> its merged intervals, kept on the host; the per-refID device table is
    // packed from it whenever the reference list or the map changes (pack_regions)
    std::unordered_map<std::string, std::vector<uint2>> regions;
    bool has_regions = false;
    uint32_t region_shift = 10;            // a grid word per 2^shift bases ($PSSBAM_REGION_GRID_SHIFT)
    std::vector<uint4> ref_info_host;      // the last set_references' table: contig length and "found" per refID, for the packing
    uint4 *d_region_info = nullptr;
    uint32_t *d_region_grid = nullptr;
    uint2 *d_region_iv = nullptr;
    // allele counts at listed sites (pssbam_engine_set_sites, allele_kernels.h): contig name -> its positions, sorted and merged,
    // kept on the host; the device table is packed from it whenever the reference list or the map changes (pack_sites).  Off:
    // nothing below is allocated and nothing more is launched.  The packed table is in the genome's order (sorted indices);
    // site_ref / site_pos / site_slot list the resolved sites in the caller's order, by refID then position, with their slot there.
    std::unordered_map<std::string, std::vector<uint32_t>> sites;
    bool has_sites = false;
    uint32_t site_trim = 0;
    uint32_t site_shift = 10;              // a grid word per 2^shift genome indices ($PSSBAM_SITE_GRID_SHIFT)
    uint64_t sites_given = 0;              // after merging
    std::vector<uint64_t> site_idx;        // the packed table's genome indices, ascending (without the closing entry)
    std::vector<int32_t> site_ref;
    std::vector<uint32_t> site_pos, site_slot;
    bool site_counts_void = false;         // a genome was set since the packing: the next one starts from zero
    uint64_t *d_site_idx = nullptr;
    uint32_t *d_site_grid = nullptr, *d_site_counts = nullptr;
    uint8_t *d_site_base = nullptr;        // finish_sites' reference letters
    uint64_t site_cells = 0;
    // counters
    unsigned long long *d_counters = nullptr;      // block in use (own or caller-bound)
    unsigned long long *d_counters_own = nullptr;  // the engine's own allocation
    size_t n_counters = 0;
    uint32_t rows = 0, off_rev = 0, off_k5 = 0, off_k3 = 0, off_stats = 0;
    uint64_t n_bins = 0;
    // staging
    Slot slots[2];
    int next_slot = 0;
    uint64_t ticket_seq = 0;
    double h2d_ms = 0.0;      // summed H2D copy durations (events on the copy stream)
    uint64_t h2d_bytes = 0;
    // device-side inflate feed
    std::vector<FeedAcc *> feed;       // ring of super-batch slots
    int cur_feed = -1, spare_feed = -1; // slot being assembled; slot acquired ahead for a submit that will spill over
    uint64_t flush_seq = 0;
    bool feed_opened = false;          // pssbam_engine_feed_open: submit_bgzf may precede set_genome / set_references
    int32_t feed_n_ref = 0;            // ... with this many references in the BAM header
    uint64_t feed_mem_budget = 0;      // device bytes the ring may take while tallies are deferred (0: not worked out yet)
    std::vector<DeferredTally> deferred;
    uint8_t *d_carry = nullptr;        // the partial record a super-batch ended with, on its way into the next slot's gap
    uint8_t *h_handoff = nullptr;      // page-locked [8 + FEED_GAP]: the partial record ANOTHER engine's run ended with arrives here (feed_handoff)
    hipEvent_t handoff_ev = nullptr;   // recorded on this engine's stream behind the hand-off of its own tail
    uint64_t feed_out_target = FEED_OUT_TARGET, feed_comp_cap = FEED_COMP_CAP;   // per super-batch
    uint64_t feed_sub_max = FEED_SUB_MAX;   // a new tally sub-batch where the record bytes would pass this ($PSSBAM_FEED_SUB_BYTES: tests)
    double feed_t_alloc = 0, feed_t_wait_busy = 0, feed_t_flush = 0;   // host seconds inside the feed (PSSBAM_STATS)
    double feed_t0 = 0, feed_t_first_flush = -1;                        // host clock of the first submit_bgzf; first flush, seconds after it
    uint64_t feed_slots_allocated = 0, feed_deferred_launches = 0, feed_early_flushes = 0;
    uint64_t feed_blocks_launched = 0, feed_lanes_launched = 0;   // blocks inflated / lanes their launches occupied (whole rounds of the kernel's grid)
    uint64_t feed_idle_min_blocks = 8192;   // a super-batch of at least so many blocks is flushed early when the device has run dry ($PSSBAM_FEED_IDLE_BLOCKS, 0 = never)
    uint64_t feed_block_target = 0;   // blocks per super-batch: a whole number of rounds of the inflate kernel's lanes
    std::vector<std::pair<uint64_t, hipEvent_t>> feed_copies;             // (ticket, copy-complete event) of submits
    std::vector<hipEvent_t> feed_event_pool;
    uint32_t *d_feed_flags = nullptr;
    uint64_t *d_feed_tail = nullptr;   // bytes of the partial record the last flushed super-batch ended with
    bool feed_fresh = true;            // nothing of the current stream has been flushed yet
    uint32_t feed_skip = 0;            // inflated bytes in front of the stream's first record (the BAM header)
    double inflate_ms = 0.0;  // summed inflate + CRC + index kernel durations
    uint64_t inflated_bytes = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> inflate_events;
    // timing
    hipEvent_t t_begin = nullptr, t_end = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> launch_events;
    std::vector<hipEvent_t> event_pool;
    double kernel_ms = 0.0;
    uint64_t kernel_launches = 0;
    // tuning overrides (environment, for experiments)
    int env_tile_reads = 0, env_grid_mult = 0, env_simple_blocks = 0, env_grid_wgs = 0, env_pieces = 0;
    int env_group_slots = 0;   // PSSBAM_GROUP_SLOTS: at most this many planes per -G launch (tests: plane passes with few groups)
    bool warned_ablate = false;
    bool compact_plan_once = false;   // tally_compact: header decode + filters once per read, plan through LDS (PSSBAM_COMPACT_PLAN_ONCE)
    std::unordered_map<const void *, KernelPrep> prep;   // tiled_grid's memo, by the kernel's host address
    bool use_compact = true;        // -r N <= 16: tally_compact (PSSBAM_COMPACT=0 keeps tally_tiled, for A/B runs)
    uint32_t *d_scratch = nullptr;  // per-workgroup partial tables of the tiled kernel
    size_t scratch_slots = 0;
    uint32_t dev_pieces = 0;       // prefix pieces sampled from a device-resident block
    uint64_t dev_pieces_avg = 0;   // ... and the mean record size it was sampled at
    // finish_coverage_windows (behind everything a submit touches, whose places stay what they were): cov_epoch counts the times the totals were computed; the windows of size cov_win_size (0: none), in
    // genome order, stand while cov_win_epoch is the epoch of totals that are still valid
    uint64_t cov_epoch = 0, cov_win_epoch = 0;
    uint32_t cov_win_size = 0;
    std::vector<unsigned long long> cov_win_sum;
    std::vector<uint32_t> cov_win_cov, cov_win_acgt, cov_win_gc;
};

static void ctx_mask(const char *set, uint32_t (&m)[8]) {
    // strchr(set, c) != NULL: every byte of the string, plus the terminator itself --
    // expressed over STORED genome bytes (enc_byte permutation, record_decode.h)
    memset(m, 0, sizeof m);
    for (const unsigned char *p = (const unsigned char *)set;; p++) {
        const uint32_t st = enc_byte(*p);
        m[st >> 5] |= 1u << (st & 31);
        if (!*p) break;
    }
}

static int env_int(const char *name) {
    const char *v = getenv(name);
    return v ? atoi(v) : 0;
}

// the streams made by the helper thread (engine struct): taken over when they are there, or -- wait -- waited for
static void late_streams(pssbam_engine *e, bool wait) {
    std::lock_guard<std::mutex> lk(e->late_mu);
    if (e->late_adopted) return;
    if (!wait && !e->late_ready.load(std::memory_order_acquire)) return;
    if (e->late_thread.joinable()) e->late_thread.join();
    e->copy_stream = e->late_copy1;
    e->copy_stream2 = e->late_copy2;
    e->genome_stream = e->late_genome;
    e->late_adopted = true;
}

extern "C" int pssbam_engine_create(const pssbam_config *cfg, pssbam_engine **out) {
    if (!cfg || !out) return fail(PSSBAM_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->abi_version != PSSBAM_ABI_VERSION)
        return fail(PSSBAM_EINVAL, "abi_version %u != %u", cfg->abi_version, PSSBAM_ABI_VERSION);
    if (!(cfg->tally_mask & (PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER)) ||
        (cfg->tally_mask & ~(PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER)))
        return fail(PSSBAM_EINVAL, "tally_mask must be a non-empty subset of PSS|KMER");
    if ((cfg->tally_mask & PSSBAM_TALLY_PSS)) {
        if (cfg->pss.region_len < 0 || cfg->pss.region_len > 1000000)
            return fail(PSSBAM_EINVAL, "region_len %d out of range", cfg->pss.region_len);
        if (!cfg->pss.up_ctx || !cfg->pss.down_ctx) return fail(PSSBAM_EINVAL, "up_ctx/down_ctx must be set");
    }
    // 4^k 64-bit bins per table in device memory: k = 15 is 2 x 8.6 GB of the 288 GB (the reference's
    // tree grows without bound, kmer.c:67-98; beyond 15 the bin index no longer fits the kernels' u32)
    if ((cfg->tally_mask & PSSBAM_TALLY_KMER) && (cfg->kmer.klen < 1 || cfg->kmer.klen > PSSBAM_MAX_KLEN))
        return fail(PSSBAM_EINVAL, "klen %d outside the device range 1..%d", cfg->kmer.klen, PSSBAM_MAX_KLEN);

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return fail(PSSBAM_ENODEV, "no HIP device available (this engine has no CPU path)");
    int dev = cfg->device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= n_dev) return fail(PSSBAM_ENODEV, "device %d does not exist (%d present)", dev, n_dev);
    if (!device_is_gfx950(dev) && !getenv("PSSBAM_ALLOW_OTHER_ARCH"))
        return fail(PSSBAM_ENODEV, "device %d is not gfx950", dev);
    HIP_TRY(hipSetDevice(dev));

    pssbam_engine *e = new pssbam_engine();
    // a failure below releases what was set up so far (destroy tolerates a half-built engine)
    std::unique_ptr<pssbam_engine, void (*)(pssbam_engine *)> guard(e, pssbam_engine_destroy);
    e->cfg = *cfg;
    e->device = dev;
    if (cfg->tally_mask & PSSBAM_TALLY_PSS) {
        e->up_ctx = cfg->pss.up_ctx;
        e->down_ctx = cfg->pss.down_ctx;
    }
    if (cfg->read_group) {
        e->rg = cfg->read_group;
        e->has_rg = true;
    }
    e->cfg.pss.up_ctx = e->cfg.pss.down_ctx = e->cfg.read_group = nullptr;
    const bool tstat = getenv("PSSBAM_STATS") != nullptr;
    const double tc0 = tstat ? feed_now() : 0.0;
    hipDeviceProp_t pr;
    HIP_TRY(hipGetDeviceProperties(&pr, dev));
    e->n_cu = pr.multiProcessorCount;
    const double tc1 = tstat ? feed_now() : 0.0;
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    if (getenv("PSSBAM_STREAMS_UP_FRONT")) {   // (A/B: all four streams before create returns, as in round 2)
        HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream2, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&e->genome_stream, hipStreamNonBlocking));
        e->late_adopted = true;
    } else {
        e->late_thread = std::thread([e, dev]() {
            if (hipSetDevice(dev) == hipSuccess) {
                if (hipStreamCreateWithFlags(&e->late_copy1, hipStreamNonBlocking) != hipSuccess) e->late_copy1 = nullptr;
                if (hipStreamCreateWithFlags(&e->late_copy2, hipStreamNonBlocking) != hipSuccess) e->late_copy2 = nullptr;
                if (hipStreamCreateWithFlags(&e->late_genome, hipStreamNonBlocking) != hipSuccess) e->late_genome = nullptr;
            }
            (void)hipGetLastError();
            e->late_ready.store(1, std::memory_order_release);
        });
    }
    HIP_TRY(hipEventCreateWithFlags(&e->genome_ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->copied2, hipEventDisableTiming));
    e->own_stream = true;
    HIP_TRY(hipEventCreate(&e->t_begin));
    HIP_TRY(hipEventCreate(&e->t_end));
    const double tc2 = tstat ? feed_now() : 0.0;

    e->rows = (cfg->tally_mask & PSSBAM_TALLY_PSS) ? (uint32_t)cfg->pss.region_len + 2u : 0u;
    e->n_bins = (cfg->tally_mask & PSSBAM_TALLY_KMER) ? (1ull << (2 * cfg->kmer.klen)) : 0ull;
    e->off_rev = e->rows * 16u;
    e->off_k5 = 2u * e->rows * 16u;
    e->off_k3 = (uint32_t)(e->off_k5 + e->n_bins);
    e->off_stats = (uint32_t)(e->off_k3 + e->n_bins);
    e->n_counters = (size_t)e->off_stats + PSSBAM_ST_N;
    e->plane_words = 2u * e->rows * 16u;
    e->off_groups = (uint32_t)e->n_counters;
    e->kplane_words = cfg->tally_mask == PSSBAM_TALLY_KMER ? 2ull * e->n_bins : 0ull;
    HIP_TRY(hipMalloc(&e->d_counters_own, e->n_counters * sizeof(unsigned long long)));
    e->d_counters = e->d_counters_own;
    HIP_TRY(hipMemsetAsync(e->d_counters, 0, e->n_counters * sizeof(unsigned long long), e->stream));
    if (e->has_rg) {
        HIP_TRY(hipMalloc(&e->d_rg, e->rg.size() + 16));
        HIP_TRY(hipMemcpy(e->d_rg, e->rg.data(), e->rg.size(), hipMemcpyHostToDevice));
    }
    for (Slot &s : e->slots) {
        HIP_TRY(hipEventCreate(&s.copy_begin));
        HIP_TRY(hipEventCreate(&s.copied));
        HIP_TRY(hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming));
    }
    // the tiled kernels' per-workgroup scratch, for the largest grid the launcher picks on its own (8 workgroups per CU): a
    // first launch that had to allocate it would first wait for everything queued on the stream -- with the compressed feed
    // running ahead of the genome that is tens of ms of inflate kernels (launch_tally)
    e->scratch_slots = (size_t)e->n_cu * 8;
    HIP_TRY(hipMalloc(&e->d_scratch, e->scratch_slots * SCRATCH_WORDS * sizeof(uint32_t)));
    e->env_tile_reads = env_int("PSSBAM_TILE_READS");
    e->env_grid_mult = env_int("PSSBAM_GRID_MULT");
    e->env_simple_blocks = env_int("PSSBAM_SIMPLE_BLOCKS");
    e->env_grid_wgs = env_int("PSSBAM_GRID_WGS");
    e->env_pieces = env_int("PSSBAM_PIECES");
    e->env_group_slots = env_int("PSSBAM_GROUP_SLOTS");
    e->env_contig_slots = env_int("PSSBAM_CONTIG_SLOTS");
    if (getenv("PSSBAM_CONTIG_EVICT")) e->contig_evict = env_int("PSSBAM_CONTIG_EVICT") != 0;
    if (getenv("PSSBAM_HIST_LDS_BINS")) e->env_hist_lds_bins = std::max(env_int("PSSBAM_HIST_LDS_BINS"), 0);
    if (const int g = env_int("PSSBAM_REGION_GRID_SHIFT")) e->region_shift = (uint32_t)std::min(std::max(g, 2), 20);
    if (const int g = env_int("PSSBAM_SITE_GRID_SHIFT")) e->site_shift = (uint32_t)std::min(std::max(g, 2), 20);
    if (getenv("PSSBAM_COMPACT")) e->use_compact = env_int("PSSBAM_COMPACT") != 0;
    if (getenv("PSSBAM_COMPACT_PLAN_ONCE")) e->compact_plan_once = env_int("PSSBAM_COMPACT_PLAN_ONCE") != 0;
    if (tstat)
        fprintf(stderr, "[pssbam] engine on device %d: device properties %.3f, its stream + events %.3f, counters + scratch (first allocations, first "
                        "enqueue) %.3f s\n", dev, tc1 - tc0, tc2 - tc1, feed_now() - tc2);
    *out = guard.release();
    return PSSBAM_OK;
}

extern "C" void pssbam_engine_destroy(pssbam_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    late_streams(e, true);
    for (hipStream_t is : e->inflate_stream)
        if (is) (void)hipStreamSynchronize(is);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
    if (e->copy_stream2) (void)hipStreamSynchronize(e->copy_stream2);
    for (Slot &s : e->slots) {
        if (s.d_recs) (void)hipFree(s.d_recs);
        if (s.d_offs) (void)hipFree(s.d_offs);
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.copy_begin) (void)hipEventDestroy(s.copy_begin);
        if (s.consumed) (void)hipEventDestroy(s.consumed);
    }
    if (e->genome_stream) (void)hipStreamSynchronize(e->genome_stream);
    for (const void *p : e->genome_pins) pin_release(p);
    e->genome_pins.clear();
    for (FeedAcc *sp : e->feed) {
        FeedAcc &s = *sp;
        void *ptrs[] = {s.d_comp, s.d_blocks, s.d_a, s.d_e, s.d_last, s.d_nexta, s.d_n, s.d_counts, s.d_base, s.d_out, s.d_offs, s.d_nrecs, s.d_chain};
        for (void *q : ptrs)
            if (q) (void)hipFree(q);
        if (s.h_blocks) (void)hipHostFree(s.h_blocks);
        if (s.consumed) (void)hipEventDestroy(s.consumed);
        if (s.copies_done) (void)hipEventDestroy(s.copies_done);
        if (s.copies_done2) (void)hipEventDestroy(s.copies_done2);
        if (s.inflated) (void)hipEventDestroy(s.inflated);
        if (s.inflate_done) (void)hipEventDestroy(s.inflate_done);
        delete sp;
    }
    e->feed.clear();
    if (e->d_carry) (void)hipFree(e->d_carry);
    if (e->h_handoff) (void)hipHostFree(e->h_handoff);
    if (e->handoff_ev) (void)hipEventDestroy(e->handoff_ev);
    for (SelectBuf &b : e->sel) {
        if (b.d_out) (void)hipFree(b.d_out);
        if (b.d_totals) (void)hipFree(b.d_totals);
        if (b.h_totals) (void)hipHostFree(b.h_totals);
        if (b.h_data) (void)hipHostFree(b.h_data);
        if (b.totals_ev) (void)hipEventDestroy(b.totals_ev);
        if (b.data_ev) (void)hipEventDestroy(b.data_ev);
    }
    if (e->sel_stream) { (void)hipStreamSynchronize(e->sel_stream); (void)hipStreamDestroy(e->sel_stream); }
    if (e->d_sel_len) (void)hipFree(e->d_sel_len);
    for (auto &p : e->dedup_old) { (void)hipFree(p.first); (void)hipEventDestroy(p.second); }
    if (e->d_dedup) (void)hipFree(e->d_dedup);
    if (e->d_dedup_slot) (void)hipFree(e->d_dedup_slot);
    if (e->d_dedup_state) (void)hipFree(e->d_dedup_state);
    if (e->h_dedup_state) (void)hipHostFree(e->h_dedup_state);
    if (e->dedup_ev) (void)hipEventDestroy(e->dedup_ev);
    for (void *q : {(void *)e->d_site_idx, (void *)e->d_site_grid, (void *)e->d_site_counts, (void *)e->d_site_base})
        if (q) (void)hipFree(q);
    if (e->d_cov) (void)hipFree(e->d_cov);
    if (e->d_cov_sums) (void)hipFree(e->d_cov_sums);
    if (e->d_cov_runcnt) (void)hipFree(e->d_cov_runcnt);
    if (e->d_cov_out) (void)hipFree(e->d_cov_out);
    if (e->d_cov_contigs) (void)hipFree(e->d_cov_contigs);
    if (e->d_cov_runs) (void)hipFree(e->d_cov_runs);
    if (e->d_sel_sums) (void)hipFree(e->d_sel_sums);
    if (e->d_comp) (void)hipFree(e->d_comp);
    if (e->d_comp_len) (void)hipFree(e->d_comp_len);
    if (e->d_comp_off) (void)hipFree(e->d_comp_off);
    for (void *q : e->retired) (void)hipFree(q);
    if (e->d_feed_tail) (void)hipFree(e->d_feed_tail);
    for (auto &p : e->feed_copies) (void)hipEventDestroy(p.second);
    for (hipEvent_t ev : e->feed_event_pool) (void)hipEventDestroy(ev);
    if (e->d_feed_flags) (void)hipFree(e->d_feed_flags);
    for (auto &p : e->inflate_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &p : e->launch_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (hipEvent_t ev : e->event_pool) (void)hipEventDestroy(ev);
    if (e->t_begin) (void)hipEventDestroy(e->t_begin);
    if (e->t_end) (void)hipEventDestroy(e->t_end);
    if (e->d_scratch) (void)hipFree(e->d_scratch);
    if (e->d_genome) (void)hipFree(e->d_genome);
    if (e->d_genome4) (void)hipFree(e->d_genome4);
    if (e->d_ref_info) (void)hipFree(e->d_ref_info);
    if (e->h_ref_info) (void)hipHostFree(e->h_ref_info);
    if (e->d_rg) (void)hipFree(e->d_rg);
    for (void *q : {(void *)e->d_region_info, (void *)e->d_region_grid, (void *)e->d_region_iv})
        if (q) (void)hipFree(q);
    if (e->d_score_w) (void)hipFree(e->d_score_w);
    if (e->d_grp_ids) (void)hipFree(e->d_grp_ids);
    if (e->d_grp_offs) (void)hipFree(e->d_grp_offs);
    if (e->d_grp_hash) (void)hipFree(e->d_grp_hash);
    if (e->d_counters_own) (void)hipFree(e->d_counters_own);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->copy_stream2) (void)hipStreamDestroy(e->copy_stream2);
    for (hipStream_t is : e->inflate_stream)
        if (is) (void)hipStreamDestroy(is);
    if (e->feed_base_ev) (void)hipEventDestroy(e->feed_base_ev);
    if (e->genome_stream) (void)hipStreamDestroy(e->genome_stream);
    if (e->genome_ready) (void)hipEventDestroy(e->genome_ready);
    if (e->copied2) (void)hipEventDestroy(e->copied2);
    delete e;
}

extern "C" int pssbam_engine_set_stream(pssbam_engine *e, void *hip_stream) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->own_stream) HIP_TRY(hipStreamDestroy(e->stream));
    e->stream = (hipStream_t)hip_stream;
    e->own_stream = false;
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// genome + references
// --------------------------------------------------------------------------------------
static constexpr uint64_t CONTIG_ALIGN = 256, CONTIG_PAD = 256;

static hipEvent_t take_event(pssbam_engine *e);
static int feed_resume(pssbam_engine *e);
static int coverage_array(pssbam_engine *e, uint64_t genome_bytes);
static void coverage_contigs(pssbam_engine *e);

// The upload still in flight (if any) has completed: its page locks go back.
static int genome_settle(pssbam_engine *e) {
    if (e->genome_pins.empty()) return PSSBAM_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(e->genome_ready));
    for (const void *p : e->genome_pins) pin_release(p);
    e->genome_pins.clear();
    return PSSBAM_OK;
}

// Lays the contigs out, allocates, and ENQUEUES copies + encode + 4-bit pack on the genome stream; tally launches wait
// for genome_ready on the device.  Nothing here waits for the engine's stream (which may be busy inflating).
static int genome_upload(pssbam_engine *e, size_t n, const char *const *ids, const uint8_t *const *seqs, const uint64_t *lens,
                         int seqs_on_device) {
    if (!e || (n && (!ids || !seqs || !lens))) return fail(PSSBAM_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc = genome_settle(e);
    if (rc) return rc;
    // sorted view, as init_genome leaves Genome.seqs (fasta-genome-io.c:236)
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return strcmp(ids[a], ids[b]) < 0; });
    std::vector<uint64_t> start(n + 1, 0);
    std::vector<uint32_t> len(n + 1, 0);
    uint64_t total = CONTIG_PAD;
    for (size_t k = 0; k < n; k++) {
        if (lens[order[k]] > 0xFFFFFF00ull)
            return fail(PSSBAM_EINVAL, "contig %s has %llu bases; the engine addresses contigs below 4 Gi bases", ids[order[k]],
                        (unsigned long long)lens[order[k]]);
        start[k] = total;
        len[k] = (uint32_t)lens[order[k]];
        total += ((uint64_t)len[k] + CONTIG_PAD + CONTIG_ALIGN - 1) / CONTIG_ALIGN * CONTIG_ALIGN;
    }
    // depth of coverage: the array for this genome's size first -- a refusal (PSSBAM_ENOMEM) leaves the genome that was set before
    // as it is; coverage then has no array, and a submit is refused until a set_genome succeeds
    if (e->coverage)
        if ((rc = coverage_array(e, total))) return rc;
    if (e->d_genome) {   // a genome is being replaced: kernels queued on the engine's stream may still read the old one
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipFree(e->d_genome));
        e->d_genome = nullptr;
        if (e->d_genome4) { HIP_TRY(hipFree(e->d_genome4)); e->d_genome4 = nullptr; }
    }
    HIP_TRY(hipMalloc(&e->d_genome, total));
    late_streams(e, true);
    if (!e->genome_stream) HIP_TRY(hipStreamCreateWithFlags(&e->genome_stream, hipStreamNonBlocking));
    hipStream_t gs = e->genome_stream;
    if (seqs_on_device) {   // the caller's device arrays were written on ITS stream (the engine's, after set_stream)
        hipEvent_t ev = take_event(e);
        if (!ev) return fail(PSSBAM_EHIP, "hipEventCreate failed");
        HIP_TRY(hipEventRecord(ev, e->stream));
        HIP_TRY(hipStreamWaitEvent(gs, ev, 0));
        e->event_pool.push_back(ev);
    }
    // padding = raw NUL, like the terminator the reference finds at index len (fragkon.c odd-k
    // windows); the encode pass below turns it into the stored form of NUL ("not a base")
    HIP_TRY(hipMemsetAsync(e->d_genome, 0, total, gs));
    // Host contigs: large ones are page-locked for the copy (cheap when the loader put them on
    // transparent huge pages: 2 MiB per pin instead of 4 KiB), which turns a staged pageable copy into
    // one DMA at link speed; if the lock is refused the plain copy below does the job.  The locks are
    // shared by the engines of the process and go back when the last upload has completed.
    const bool try_lock = !seqs_on_device && !getenv("PSSBAM_NO_PIN");
    for (size_t k = 0; k < n; k++) {
        if (!len[k]) continue;
        const void *src = seqs[order[k]];
        if (try_lock && len[k] >= (32u << 20) && pin_acquire(src, len[k])) e->genome_pins.push_back(src);
        HIP_TRY(hipMemcpyAsync(e->d_genome + start[k], src, len[k],
                               seqs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, gs));
    }
    // raw bytes (and NUL padding) are in place: one pass folds case and applies enc_byte to all
    hipLaunchKernelGGL(encode_genome_kernel, dim3(4096), dim3(256), 0, gs, e->d_genome, total / 16);
    HIP_TRY(hipGetLastError());
    {
        // 4 bits per base for the tiled kernel's windows: A C G T, or "other" with its -U / -D membership
        CtxSets sets;
        ctx_mask(e->up_ctx.c_str(), sets.up);
        ctx_mask(e->down_ctx.c_str(), sets.down);
        e->acgt_ctx = 0;
        for (uint32_t v = 0; v < 4; v++)
            e->acgt_ctx |= (((sets.up[0] >> v) & 1u) << (2 * v)) | (((sets.down[0] >> v) & 1u) << (2 * v + 1));
        const uint64_t n_out = total / 8, slack = 16;
        HIP_TRY(hipMalloc(&e->d_genome4, (n_out + slack) * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(e->d_genome4 + n_out, 0x44, slack * sizeof(uint32_t), gs));
        hipLaunchKernelGGL(pack_genome4_kernel, dim3(4096), dim3(256), 0, gs, e->d_genome, e->d_genome4, n_out, sets);
        HIP_TRY(hipGetLastError());
    }
    // depth of coverage: zeroed on the genome's stream (every tally waits for genome_ready; kernels of an earlier genome that
    // added to it on the engine's stream have been waited for above, where that genome was freed)
    if (e->coverage) HIP_TRY(hipMemsetAsync(e->d_cov, 0, e->cov_len * sizeof(uint32_t), gs));
    e->site_counts_void = true;   // allele counts: the table packed for the genome before counts nothing of this one
    HIP_TRY(hipEventRecord(e->genome_ready, gs));
    e->genome_wait_pending = true;
    e->contig_start.assign(start.begin(), start.begin() + n);
    e->contig_len.assign(len.begin(), len.begin() + n);
    e->genome_bytes = total;
    e->contig_ids.clear();
    for (size_t k = 0; k < n; k++) e->contig_ids.emplace_back(ids[order[k]]);
    e->star_contig = -1;
    if (e->have_refs) e->have_refs = false;   // (written only when it changes: another thread may be feeding, see pssbam_hip.h)
    {   // RNAME "*" (refID -1) goes through find_seq like any other name
        auto it = std::lower_bound(e->contig_ids.begin(), e->contig_ids.end(), std::string("*"),
                                   [](const std::string &a, const std::string &b) { return strcmp(a.c_str(), b.c_str()) < 0; });
        if (it != e->contig_ids.end() && *it == "*") e->star_contig = (int32_t)(it - e->contig_ids.begin());
    }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_genome_arrays(pssbam_engine *e, size_t n, const char *const *ids,
                                               const uint8_t *const *seqs, const uint64_t *lens,
                                               int seqs_on_device) {
    int rc = genome_upload(e, n, ids, seqs, lens, seqs_on_device);
    if (rc) return rc;
    if (e->genome_stream) HIP_TRY(hipStreamSynchronize(e->genome_stream));   // the caller may release its arrays when this returns
    return genome_settle(e);
}

static int genome_from_struct(pssbam_engine *e, const struct genome *g, bool wait) {
    if (!e || !g) return fail(PSSBAM_EINVAL, "null argument");
    std::vector<const char *> ids(g->n_seqs);
    std::vector<const uint8_t *> seqs(g->n_seqs);
    std::vector<uint64_t> lens(g->n_seqs);
    for (size_t i = 0; i < g->n_seqs; i++) {
        ids[i] = g->seqs[i]->id;
        seqs[i] = (const uint8_t *)g->seqs[i]->seq;
        lens[i] = g->seqs[i]->len;
    }
    return wait ? pssbam_engine_set_genome_arrays(e, g->n_seqs, ids.data(), seqs.data(), lens.data(), 0)
                : genome_upload(e, g->n_seqs, ids.data(), seqs.data(), lens.data(), 0);
}

extern "C" int pssbam_engine_set_genome(pssbam_engine *e, const struct genome *g) { return genome_from_struct(e, g, true); }

// Same, but returns as soon as the upload is enqueued: the Genome must stay untouched until pssbam_engine_genome_wait,
// _sync or _finish has returned.  Lets one host thread start the uploads of several GPUs at once.
extern "C" int pssbam_engine_set_genome_async(pssbam_engine *e, const struct genome *g) { return genome_from_struct(e, g, false); }

extern "C" int pssbam_engine_genome_wait(pssbam_engine *e) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    if (e->genome_stream) HIP_TRY(hipStreamSynchronize(e->genome_stream));
    return genome_settle(e);
}

// -T: packs the per-refID region table for the current reference list (ref_names / ref_info_host) on the device:
// the descriptors, every listed contig's intervals with their ends clamped to the contig, and a grid per contig that
// has intervals (record_decode.h: TallyParams::region_*).  Plain device memory written by hipMemcpy.  `in_use`: queued
// kernels may still read the previous table (SAM text: the reference list grows), so the stream is drained first.
static int pack_regions(pssbam_engine *e, bool in_use) {
    if (!e->has_regions) return PSSBAM_OK;
    const size_t n_ent = (size_t)e->n_ref + 1;
    const uint32_t g = e->region_shift;
    std::vector<uint4> desc(n_ent, make_uint4(0, 0, 0, 0));
    // sizes first, in 64 bits
    uint64_t n_iv = 0, n_grid = 0;
    std::vector<const std::vector<uint2> *> src(n_ent, nullptr);
    for (size_t i = 0; i < n_ent; i++) {
        const uint4 ri = e->ref_info_host[i];
        if (!ri.w) continue;   // the genome lacks the name: its records are never candidates
        const auto it = e->regions.find(i < (size_t)e->n_ref ? e->ref_names[i] : std::string("*"));
        if (it == e->regions.end()) continue;
        uint64_t cnt = 0;
        for (const uint2 &v : it->second) cnt += v.x < ri.z ? 1u : 0u;   // (ascending: the ones inside the contig lead)
        if (!cnt) continue;
        src[i] = &it->second;
        desc[i] = make_uint4(0, (uint32_t)cnt, 0, 0);
        n_iv += cnt;
        n_grid += ((uint64_t)ri.z >> g) + 2;
    }
    if (n_iv >= (1ull << 32) || n_grid >= (1ull << 32)) return fail(PSSBAM_ENOMEM, "the region table has too many intervals or grid words for 32-bit indices");
    const uint64_t bytes = n_ent * sizeof(uint4) + (n_iv + 1) * sizeof(uint2) + (n_grid + 2) * sizeof(uint32_t);
    HIP_TRY(hipSetDevice(e->device));
    if (in_use && e->d_region_info) HIP_TRY(hipStreamSynchronize(e->stream));
    for (void **q : {(void **)&e->d_region_info, (void **)&e->d_region_grid, (void **)&e->d_region_iv})
        if (*q) { HIP_TRY(hipFree(*q)); *q = nullptr; }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes > (uint64_t)free_b)
        return fail(PSSBAM_ENOMEM, "the region table (%llu intervals, grid shift %u) needs %llu bytes; the device has %llu free",
                    (unsigned long long)n_iv, g, (unsigned long long)bytes, (unsigned long long)free_b);
    std::vector<uint2> iv((size_t)n_iv + 1, make_uint2(0, 0));
    std::vector<uint32_t> grid((size_t)n_grid + 2, 0u);
    uint64_t at_iv = 0, at_grid = 0;
    for (size_t i = 0; i < n_ent; i++) {
        if (!src[i]) continue;
        const uint32_t len = e->ref_info_host[i].z, cnt = desc[i].y;
        desc[i].x = (uint32_t)at_iv;
        desc[i].z = (uint32_t)at_grid;
        uint2 *out = iv.data() + at_iv;
        for (uint32_t k = 0; k < cnt; k++) out[k] = make_uint2((*src[i])[k].x, std::min((*src[i])[k].y, len));
        // grid[b] = first interval whose end lies beyond b << g; one closing word = cnt
        const uint64_t n_bins = ((uint64_t)len >> g) + 1;
        uint32_t j = 0;
        for (uint64_t b = 0; b < n_bins; b++) {
            while (j < cnt && (uint64_t)out[j].y <= (b << g)) j++;
            grid[at_grid + b] = j;
        }
        grid[at_grid + n_bins] = cnt;
        at_iv += cnt;
        at_grid += n_bins + 1;
    }
    HIP_TRY(hipMalloc(&e->d_region_info, n_ent * sizeof(uint4)));
    HIP_TRY(hipMalloc(&e->d_region_iv, iv.size() * sizeof(uint2)));
    HIP_TRY(hipMalloc(&e->d_region_grid, grid.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(e->d_region_info, desc.data(), n_ent * sizeof(uint4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_region_iv, iv.data(), iv.size() * sizeof(uint2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_region_grid, grid.data(), grid.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_regions(pssbam_engine *e, int32_t n_names, const char *const *names, int64_t n_regions,
                                         const int32_t *name_of, const uint32_t *starts, const uint32_t *ends) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (n_names < 0 || n_regions < 0 || n_regions > PSSBAM_MAX_REGIONS) return fail(PSSBAM_EINVAL, "region count outside 0..%d", PSSBAM_MAX_REGIONS);
    if ((n_names && !names) || (n_regions && (!name_of || !starts || !ends))) return fail(PSSBAM_EINVAL, "null region list");
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set the regions after create or reset, before the first tally");
    std::unordered_map<std::string, std::vector<uint2>> map;
    for (int32_t k = 0; k < n_names; k++) {
        if (!names[k]) return fail(PSSBAM_EINVAL, "region contig name %d is NULL", k);
        if (n_regions) map[names[k]];   // listed, perhaps with nothing: tallies nothing
    }
    for (int64_t i = 0; i < n_regions; i++) {
        if (name_of[i] < 0 || name_of[i] >= n_names) return fail(PSSBAM_EINVAL, "region %lld: contig index %d outside 0..%d", (long long)i, name_of[i], n_names - 1);
        if (starts[i] > ends[i])
            return fail(PSSBAM_EINVAL, "region %lld on %s: start %u lies behind end %u", (long long)i, names[name_of[i]], starts[i], ends[i]);
        if (starts[i] < ends[i]) map[names[name_of[i]]].push_back(make_uint2(starts[i], ends[i]));   // (an empty interval is dropped)
    }
    for (auto &kv : map) {   // sorted, then overlapping, nested and touching intervals merged: disjoint, non-adjacent, ascending
        std::vector<uint2> &v = kv.second;
        std::sort(v.begin(), v.end(), [](const uint2 &a, const uint2 &b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
        size_t n = 0;
        for (const uint2 &r : v) {
            if (n && r.x <= v[n - 1].y) v[n - 1].y = std::max(v[n - 1].y, r.y);
            else v[n++] = r;
        }
        v.resize(n);
    }
    HIP_TRY(hipSetDevice(e->device));
    e->regions.swap(map);
    e->has_regions = n_regions > 0;
    if (!e->has_regions) {   // switched off: the engine launches what it launches without the call
        if (e->d_region_info) HIP_TRY(hipStreamSynchronize(e->stream));
        for (void **q : {(void **)&e->d_region_info, (void **)&e->d_region_grid, (void **)&e->d_region_iv})
            if (*q) { HIP_TRY(hipFree(*q)); *q = nullptr; }
        return PSSBAM_OK;
    }
    return e->have_refs ? pack_regions(e, true) : PSSBAM_OK;   // (otherwise set_references packs the table when it comes)
}

// Allele counts: packs the site table for the current reference list (ref_names / ref_info_host) and genome on the device: the
// resolved sites as sorted genome indices with a closing entry, the grid over them and the counters (allele_kernels.h).  A name
// no reference carries, a position at or beyond the contig's stored length and the later of two references of one name are
// dropped.  Counters of a table that has counted (SAM text: the reference list grows while blocks are tallied) move to the new
// table by genome index; after create, reset or a new genome they start from zero.
static void free_sites(pssbam_engine *e) {
    for (void **q : {(void **)&e->d_site_idx, (void **)&e->d_site_grid, (void **)&e->d_site_counts, (void **)&e->d_site_base})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
    e->site_cells = 0;
}

static int pack_sites(pssbam_engine *e) {
    if (!e->has_sites) return PSSBAM_OK;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> old_counts;
    std::vector<uint64_t> old_idx;
    if (e->d_site_idx) {   // queued kernels may still add to the table that is replaced
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->tallied && !e->site_counts_void && !e->site_idx.empty()) {
            old_counts.resize(e->site_idx.size() * ALLELE_WORDS);
            HIP_TRY(hipMemcpy(old_counts.data(), e->d_site_counts, old_counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            old_idx.swap(e->site_idx);
        }
        free_sites(e);
    }
    e->site_counts_void = false;
    e->site_idx.clear();
    e->site_ref.clear();
    e->site_pos.clear();
    e->site_slot.clear();
    std::unordered_set<uint64_t> seen;   // the contigs met so far, by their place in the genome
    for (size_t i = 0; i < (size_t)e->n_ref; i++) {   // (the entry behind them answers RNAME "*": no site is listed there)
        const uint4 ri = e->ref_info_host[i];
        if (!ri.w) continue;   // the genome lacks the name
        const auto it = e->sites.find(e->ref_names[i]);
        if (it == e->sites.end()) continue;
        const uint64_t lo = ((uint64_t)ri.y << 32) | ri.x;
        if (!seen.insert(lo).second) continue;   // the later of two references of one name
        for (const uint32_t p : it->second) {   // (ascending: the ones inside the contig lead)
            if (p >= ri.z) break;
            e->site_ref.push_back((int32_t)i);
            e->site_pos.push_back(p);
            e->site_idx.push_back(lo + p);
        }
    }
    const size_t n = e->site_idx.size();
    if (!n) return PSSBAM_OK;   // nothing resolved: nothing allocated, nothing launched
    std::vector<uint32_t> order(n);
    for (size_t j = 0; j < n; j++) order[j] = (uint32_t)j;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return e->site_idx[a] < e->site_idx[b]; });
    std::vector<uint64_t> idx(n + 1);
    e->site_slot.assign(n, 0u);
    for (size_t k = 0; k < n; k++) {
        idx[k] = e->site_idx[order[k]];
        e->site_slot[order[k]] = (uint32_t)k;
    }
    idx[n] = ~0ull;
    e->site_idx.assign(idx.begin(), idx.begin() + (ptrdiff_t)n);
    // grid[c] = the first site at or after c << shift; one closing word = n
    const uint32_t g = e->site_shift;
    const uint64_t n_cells = (e->genome_bytes >> g) + 1;
    std::vector<uint32_t> grid((size_t)n_cells + 1);
    {
        size_t k = 0;
        for (uint64_t c = 0; c <= n_cells; c++) {
            while (k < n && idx[k] < (c << g)) k++;
            grid[(size_t)c] = (uint32_t)k;
        }
    }
    std::vector<uint32_t> counts(n * ALLELE_WORDS, 0u);
    for (size_t k = 0, o = 0; k < n && o < old_idx.size(); k++) {   // both ascending
        while (o < old_idx.size() && old_idx[o] < idx[k]) o++;
        if (o < old_idx.size() && old_idx[o] == idx[k]) memcpy(&counts[k * ALLELE_WORDS], &old_counts[o * ALLELE_WORDS], ALLELE_WORDS * sizeof(uint32_t));
    }
    if (hipMalloc((void **)&e->d_site_idx, idx.size() * sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&e->d_site_grid, grid.size() * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&e->d_site_counts, counts.size() * sizeof(uint32_t)) != hipSuccess || hipMalloc((void **)&e->d_site_base, n) != hipSuccess) {
        (void)hipGetLastError();
        free_sites(e);
        e->site_idx.clear();
        e->site_ref.clear();
        e->site_pos.clear();
        e->site_slot.clear();
        return fail(PSSBAM_ENOMEM, "the site table (%llu sites, %llu grid words at shift %u) does not fit the device", (unsigned long long)n,
                    (unsigned long long)grid.size(), g);
    }
    e->site_cells = n_cells;
    HIP_TRY(hipMemcpy(e->d_site_idx, idx.data(), idx.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_site_grid, grid.data(), grid.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_site_counts, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_sites(pssbam_engine *e, int32_t n_names, const char *const *names, int64_t n_sites, const int32_t *name_of,
                                       const uint32_t *pos0, uint32_t trim) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (n_names < 0 || n_sites < 0 || n_sites > PSSBAM_MAX_REGIONS) return fail(PSSBAM_EINVAL, "site count outside 0..%d", PSSBAM_MAX_REGIONS);
    if (trim > PSSBAM_MAX_SITE_TRIM) return fail(PSSBAM_EINVAL, "site trim %u above %d", trim, PSSBAM_MAX_SITE_TRIM);
    if ((n_names && !names) || (n_sites && (!name_of || !pos0))) return fail(PSSBAM_EINVAL, "null site list");
    if (n_sites) {
        if (!(e->cfg.tally_mask & PSSBAM_TALLY_PSS)) return fail(PSSBAM_EINVAL, "the sites count the bases of the reads in the substitution tables: the engine needs PSSBAM_TALLY_PSS");
        if (e->gapped) return fail(PSSBAM_EINVAL, "sites do not go with gapped reads (pssbam_engine_set_gapped_reads): the offsets of a clipped or gapped read need a CIGAR walk");
    }
    if (e->tallied || e->cur_feed >= 0 || !e->deferred.empty())
        return fail(PSSBAM_ESTATE, "records have been tallied already: set the sites after create or reset, before the first submit");
    std::unordered_map<std::string, std::vector<uint32_t>> map;
    for (int64_t i = 0; i < n_sites; i++) {
        if (name_of[i] < 0 || name_of[i] >= n_names) return fail(PSSBAM_EINVAL, "site %lld: contig index %d outside 0..%d", (long long)i, name_of[i], n_names - 1);
        if (!names[name_of[i]]) return fail(PSSBAM_EINVAL, "site contig name %d is NULL", name_of[i]);
        map[names[name_of[i]]].push_back(pos0[i]);
    }
    uint64_t given = 0;
    for (auto &kv : map) {   // sorted, duplicates merged
        std::vector<uint32_t> &v = kv.second;
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        given += v.size();
    }
    HIP_TRY(hipSetDevice(e->device));
    e->sites.swap(map);
    e->has_sites = n_sites > 0;
    e->site_trim = trim;
    e->sites_given = given;
    if (!e->has_sites) {   // switched off: nothing stays allocated, the engine launches what it launches without the call
        if (e->d_site_idx) HIP_TRY(hipStreamSynchronize(e->stream));
        free_sites(e);
        e->site_idx.clear();
        e->site_ref.clear();
        e->site_pos.clear();
        e->site_slot.clear();
        return PSSBAM_OK;
    }
    return e->have_refs ? pack_sites(e) : PSSBAM_OK;   // (otherwise set_references packs the table when it comes)
}

static int size_per_contig(pssbam_engine *e, int32_t n_ref);

extern "C" int pssbam_engine_set_references(pssbam_engine *e, int32_t n_ref, const char *const *names) {
    if (!e || n_ref < 0 || (n_ref && !names)) return fail(PSSBAM_EINVAL, "bad argument");
    if (!e->d_genome) return fail(PSSBAM_ESTATE, "set_genome must precede set_references");
    HIP_TRY(hipSetDevice(e->device));
    // ref_info[i] = {gbase lo, gbase hi, length, found | plane << 1}; entry n_ref answers RNAME "*" (refID -1).
    // plane = 1 + the -C set that lists the name (0: none); a name the genome lacks stays all zero.
    std::vector<uint4> info((size_t)n_ref + 1, make_uint4(0, 0, 0, 0));
    auto fill = [&](size_t slot, int32_t contig, const char *name) {
        if (contig < 0) return;
        const uint64_t gb = e->contig_start[(size_t)contig];
        uint32_t plane = 0;
        if (!e->ctg_plane.empty()) {
            const auto it = e->ctg_plane.find(name);
            if (it != e->ctg_plane.end()) plane = it->second;
        }
        info[slot] = make_uint4((uint32_t)gb, (uint32_t)(gb >> 32), e->contig_len[(size_t)contig], 1u | plane << 1);
    };
    for (int32_t i = 0; i < n_ref; i++) {
        // bsearch with strcmp over the sorted ids == find_seq (fasta-genome-io.c:202-213)
        size_t lo = 0, hi = e->contig_ids.size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            const int c = strcmp(names[i], e->contig_ids[mid].c_str());
            if (c == 0) { fill((size_t)i, (int32_t)mid, names[i]); break; }
            if (c < 0) hi = mid; else lo = mid + 1;
        }
    }
    fill((size_t)n_ref, e->star_contig, "*");
    // what can refuse the call comes before anything of the engine changes
    if (e->feed_opened && !e->deferred.empty() && n_ref != e->feed_n_ref)
        return fail(PSSBAM_ESTATE, "pssbam_engine_feed_open announced %d references, set_references brings %d", e->feed_n_ref, n_ref);
    if (e->per_contig)   // -A: a plane per reference (and one for "*")
        if (const int rc = size_per_contig(e, n_ref)) return rc;
    e->ref_names.assign(names, names + n_ref);   // for a pssbam_engine_set_contig_sets / _set_regions after this call
    // a table that is being REPLACED (SAM text: the list grows as new RNAMEs show up) may still be read by queued
    // kernels; the first one cannot be, so nothing waits for the engine's stream then
    if (e->d_ref_info) {
        if (e->have_refs) HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipFree(e->d_ref_info));
        e->d_ref_info = nullptr;
    }
    HIP_TRY(hipMalloc(&e->d_ref_info, ((size_t)n_ref + 1) * sizeof(uint4)));
    // The table is a few hundred bytes, but a hipMemcpy of it queues behind whatever the copy engines are moving -- the 3 GB
    // genome, typically: 50 ms during which the calling thread feeds nothing.  It goes through page-locked host memory
    // instead and a one-workgroup kernel on the engine's stream reads it from there (ordered in front of every tally).
    if (e->h_ref_cap < (size_t)n_ref + 1) {
        if (e->h_ref_info) (void)hipHostFree(e->h_ref_info);
        e->h_ref_info = nullptr;
        e->h_ref_cap = (size_t)n_ref + 1 + 64;
        HIP_TRY(hipHostMalloc((void **)&e->h_ref_info, e->h_ref_cap * sizeof(uint4), hipHostMallocDefault));
    } else if (e->have_refs) HIP_TRY(hipStreamSynchronize(e->stream));   // (a kernel may still be reading the previous contents)
    memcpy(e->h_ref_info, info.data(), ((size_t)n_ref + 1) * sizeof(uint4));
    hipLaunchKernelGGL(copy_table_kernel, dim3(1), dim3(256), 0, e->stream, e->d_ref_info, (const uint4 *)e->h_ref_info, (uint32_t)n_ref + 1u);
    HIP_TRY(hipGetLastError());
    const bool replaced = e->have_refs;
    e->n_ref = n_ref;
    e->have_refs = true;
    e->ref_info_host.swap(info);
    coverage_contigs(e);   // depth of coverage: the list its finish kernels find a position's contig in
    if (const int rc = pack_regions(e, replaced)) return rc;   // -T: the region table follows the reference list
    if (const int rc = pack_sites(e)) return rc;               // the site table too
    return feed_resume(e);   // super-batches inflated ahead of the genome are tallied now
}

// --------------------------------------------------------------------------------------
// launch
// --------------------------------------------------------------------------------------
static hipEvent_t take_event(pssbam_engine *e) {
    if (!e->event_pool.empty()) {
        hipEvent_t ev = e->event_pool.back();
        e->event_pool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
}

static int resolve_launch_events(pssbam_engine *e) {
    for (auto &p : e->launch_events) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(p.second));
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        e->kernel_ms += ms;
        e->kernel_launches++;
        e->event_pool.push_back(p.first);
        e->event_pool.push_back(p.second);
    }
    e->launch_events.clear();
    return PSSBAM_OK;
}

// Grid of one launch of a tiled-family kernel over n_tiles tiles: n_cu x occupancy x PSSBAM_GRID_MULT workgroups
// (PSSBAM_GRID_WGS: that many), at most one per tile; d_scratch grows to `words` per workgroup.  The kernel's
// dynamic-LDS limit and occupancy are remembered per kernel and set again only when its LDS size changes, so the steady
// state makes no runtime API calls per launch beyond the launches themselves.
template <class K>
static int tiled_grid(pssbam_engine *e, K kernel, uint32_t lds, uint32_t n_tiles, uint32_t words, uint32_t *grid) {
    KernelPrep &prep = e->prep[(const void *)kernel];
    if (prep.lds != lds || prep.occ < 1) {
        int occ = 0;
        HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, TILED_THREADS, lds));
        if (occ < 1) return fail(PSSBAM_EHIP, "kernel does not fit a CU with %u bytes of LDS", lds);
        prep.lds = lds;
        prep.occ = occ;
    }
    const int mult = e->env_grid_mult > 0 ? e->env_grid_mult : 1;
    *grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)e->n_cu * prep.occ * mult);
    if (e->env_grid_wgs > 0) *grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)e->env_grid_wgs);
    const size_t need_slots = ((size_t)*grid * words + SCRATCH_WORDS - 1) / SCRATCH_WORDS;
    if (e->scratch_slots < need_slots) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->d_scratch) HIP_TRY(hipFree(e->d_scratch));
        e->d_scratch = nullptr;
        e->scratch_slots = need_slots;
        HIP_TRY(hipMalloc(&e->d_scratch, e->scratch_slots * SCRATCH_WORDS * sizeof(uint32_t)));
    }
    return PSSBAM_OK;
}

// One launch of a tiled-family tally kernel and of the reduce kernel that sums the `words` of scratch each of its workgroups
// leaves into the counter block: kernel(P, planes...), then reduce(P, planes..., workgroups, tail...)
template <class K, class R, class... Planes, class... Tail>
static int launch_with_reduce(pssbam_engine *e, K kernel, R reduce, uint32_t words, uint32_t lds, uint32_t n_tiles, TallyParams &P,
                              const std::tuple<Planes...> &planes, Tail... tail) {
    uint32_t grid = 0;
    const int rc = tiled_grid(e, kernel, lds, n_tiles, words, &grid);
    if (rc != PSSBAM_OK) return rc;
    P.scratch = e->d_scratch;
    std::apply([&](const auto &...G) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(TILED_THREADS), lds, e->stream, P, G...);
        hipLaunchKernelGGL(reduce, dim3((words * REDUCE_GROUPS + 255) / 256), dim3(256), 0, e->stream, P, G..., grid, tail...);
    }, planes);
    return PSSBAM_OK;
}

// f(std::bool_constant<flag>...): runtime flags turned into template arguments
template <class F>
static int with_flags(F f) { return f(); }
template <class F, class... Flags>
static int with_flags(F f, bool flag, Flags... rest) {
    return flag ? with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
                : with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// f(std::integral_constant<PlaneSel, sel>): the same for the plane selector of an engine with planes
template <class F>
static int with_planes(PlaneSel sel, F f) {
    return sel == PLANES_RG    ? f(std::integral_constant<PlaneSel, PLANES_RG>{})
           : sel == PLANES_LEN ? f(std::integral_constant<PlaneSel, PLANES_LEN>{})
           : sel == PLANES_HASH ? f(std::integral_constant<PlaneSel, PLANES_HASH>{})
                               : f(std::integral_constant<PlaneSel, PLANES_REF>{});
}

static int no_kernel() { return fail(PSSBAM_EINVAL, "no tally kernel is built for this combination of options"); }

// f(std::integral_constant<TallyArm, arm>): and for the arm of a tally_tiled launch
template <class F>
static int with_arm(TallyArm arm, F f) {
    return arm == ARM_HIST       ? f(std::integral_constant<TallyArm, ARM_HIST>{})
           : arm == ARM_SITE     ? f(std::integral_constant<TallyArm, ARM_SITE>{})
           : arm == ARM_END      ? f(std::integral_constant<TallyArm, ARM_END>{})
           : arm == ARM_GAPPED   ? f(std::integral_constant<TallyArm, ARM_GAPPED>{})
           : arm == ARM_MISM     ? f(std::integral_constant<TallyArm, ARM_MISM>{})
           : arm == ARM_INTERIOR ? f(std::integral_constant<TallyArm, ARM_INTERIOR>{})
           : arm == ARM_COMP     ? f(std::integral_constant<TallyArm, ARM_COMP>{})
           : arm == ARM_SCORE    ? f(std::integral_constant<TallyArm, ARM_SCORE>{})
                                 : f(std::integral_constant<TallyArm, ARM_NONE>{});
}

static bool mismatches_on(const pssbam_engine *e) { return e->mism_hist > 0 || e->mism_max >= 0; }   // -n / -N
static bool interior_on(const pssbam_engine *e) { return e->interior_margin >= 0; }   // -W
static bool composition_on(const pssbam_engine *e) { return e->composition > 0; }   // -P
static bool read_score_on(const pssbam_engine *e) { return e->d_score_w != nullptr; }   // -y / -Y

// The exclusive modes: at most one is on in an engine.  Their extra counter words all start at off_groups, and the ones that
// take a read's fate from the whole read do so in the one 32-row pass.  `arm` is the arm of tally_tiled that computes the mode
// (the plane modes have kernels of their own).  A new mode is one row here.
enum Mode { MODE_RG, MODE_LEN, MODE_REF, MODE_HASH, MODE_EACH, MODE_HIST, MODE_SITE, MODE_END, MODE_GAPPED, MODE_MISM, MODE_INTERIOR,
            MODE_COMPOSITION, MODE_SCORE };
static const struct { const char *name; bool (*on)(const pssbam_engine *); TallyArm arm; } MODES[] = {
    {"read groups", [](const pssbam_engine *e) { return e->planes == PLANES_RG; }, ARM_NONE},
    {"length bins", [](const pssbam_engine *e) { return e->planes == PLANES_LEN; }, ARM_NONE},
    {"contig sets", [](const pssbam_engine *e) { return e->planes == PLANES_REF; }, ARM_NONE},
    {"replicates", [](const pssbam_engine *e) { return e->planes == PLANES_HASH; }, ARM_NONE},
    {"per-contig tables", [](const pssbam_engine *e) { return e->per_contig; }, ARM_NONE},
    {"the length histogram", [](const pssbam_engine *e) { return e->hist_max > 0; }, ARM_HIST},
    {"site context", [](const pssbam_engine *e) { return e->site_mode != PSSBAM_SITE_NONE; }, ARM_SITE},
    {"the end condition", [](const pssbam_engine *e) { return e->end_depth > 0; }, ARM_END},
    {"gapped reads", [](const pssbam_engine *e) { return e->gapped; }, ARM_GAPPED},
    {"the mismatch count", mismatches_on, ARM_MISM},
    {"the interior table", interior_on, ARM_INTERIOR},
    {"the composition table", composition_on, ARM_COMP},
    {"the read score", read_score_on, ARM_SCORE},
};

// The arm of the engine's tally_tiled launches: that of the mode that is on
static TallyArm tally_arm(const pssbam_engine *e) {
    for (const auto &m : MODES)
        if (m.on(e)) return m.arm;
    return ARM_NONE;
}

// One row pass of tally_tiled and its reduce_partials: the instantiation for the launch's tallies, the pass (LATER: rows
// 32.. of a large -r), its -Q and -T state and its arm.  Which instantiations there are says tally_tiled_exists
// (tally_kernels.h).  (ARM_SITE, ARM_END: the larger scratch slot of the -X / -E instantiations and the reduce that walks it)
static int launch_tiled(pssbam_engine *e, TallyParams &P, bool do_pss, bool do_kmer, bool kmer_lds, bool later, bool maskq, bool regions,
                        TallyArm arm, uint32_t lds, uint32_t n_tiles) {
    return with_arm(arm, [&](auto ARM) -> int {
        return with_flags([&](auto DO_PSS, auto DO_KMER, auto LDS_KMER, auto LATER, auto MASKQ, auto REGIONS) -> int {
            if constexpr (tally_tiled_exists(DO_PSS(), DO_KMER(), LDS_KMER(), LATER(), MASKQ(), ARM()))
                return launch_with_reduce(e, tally_tiled<DO_PSS(), DO_KMER(), LDS_KMER(), LATER(), MASKQ(), REGIONS(), ARM()>,
                                          reduce_partials<ARM() == ARM_SITE, ARM() == ARM_END>,
                                          ARM() == ARM_SITE ? SITE_SCRATCH_WORDS : ARM() == ARM_END ? END_SCRATCH_WORDS : SCRATCH_WORDS, lds, n_tiles, P,
                                          std::tuple<>(), (uint32_t)LDS_KMER());
            else
                return no_kernel();
        }, do_pss, do_kmer, kmer_lds, later, maskq, regions);
    });
}


// How many 16-byte pieces of a record the tiled kernel must stage so that everything the path
// reads (through QUAL[0]; the whole record when the -R filter walks the aux fields) is in LDS
// for typical records: sampled from the first records of a block.  Records that need more take
// the kernel's out-of-line global-memory path, so this is a performance choice only.
// (returns the largest prefix, in bytes, any sampled record needs)
static uint64_t sample_prefix_need(const uint8_t *bytes, uint64_t nbytes, bool whole_record, int max_records = 4096) {
    uint64_t o = 0, need_max = 64;
    for (int n = 0; n < max_records && o + 36 <= nbytes; n++) {
        uint32_t bs, l_seq;
        memcpy(&bs, bytes + o, 4);
        if (bs < 32 || o + 4 + (uint64_t)bs > nbytes) break;
        const uint32_t l_name = bytes[o + 12];
        uint16_t n_cig;
        memcpy(&n_cig, bytes + o + 16, 2);
        memcpy(&l_seq, bytes + o + 20, 4);
        const uint64_t qual_off = 36ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2;
        const uint64_t need = whole_record ? 4ull + bs : std::min<uint64_t>(qual_off + 1, 4ull + bs);
        need_max = std::max(need_max, need);
        o += 4 + (uint64_t)bs;
    }
    return need_max;
}

// -R and -G walk the aux fields, which sit behind QUAL, and -Q and -y / -Y read QUAL itself: the tiled kernels stage whole records
static bool whole_records(const pssbam_engine *e) { return e->has_rg || e->planes == PLANES_RG || e->min_bq > 0 || e->d_score_w != nullptr; }

// The plane kernels' argument for the engine's -G / -S state (plane0, n_slots and scratch_words are per launch)
static PlaneParams plane_params(const pssbam_engine *e) {
    PlaneParams G{};
    G.ids = e->d_grp_ids;
    G.id_offs = e->d_grp_offs;
    G.hash = e->d_grp_hash;
    G.hash_mask = e->grp_hash_mask;
    G.n_groups = e->n_planes;
    G.n_slots = e->n_planes + 1u;
    G.plane_words = e->plane_words;
    G.off_groups = e->off_groups;
    G.koff_planes = e->off_groups;
    G.kplane_words = e->kplane_words;
    G.n_edges = (uint32_t)e->len_edges.size();
    std::copy(e->len_edges.begin(), e->len_edges.end(), G.edges);
    return G;
}

static uint32_t pieces_for(uint64_t need_max) {
    uint64_t pieces = (need_max + 15 + 15) / 16;  // + worst-case misalignment of the record start
    // records sit pieces*16 bytes apart in LDS: an even piece count puts every record start of a
    // wave on few banks (pieces = 8 -> all on one); an odd count spreads them over 8
    pieces |= 1;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pieces, 5), 41);
}

// --------------------------------------------------------------------------------------
// the record sink: mark, scan, gather behind a tally launch; totals, then data, to the host; delivery in order
// --------------------------------------------------------------------------------------
static uint64_t select_reserve_bytes(const pssbam_engine *e);   // (bgzf_api.h: what the sink's buffers take from the feed's memory budget)

// (bgzf_api.h) deflate + scan + pack of a stream of at most max_bytes bytes, *d_total of them
static int launch_deflate(hipStream_t st, const uint8_t *d_raw, uint64_t max_bytes, const unsigned long long *d_total, uint8_t *d_comp,
                          uint32_t *d_comp_len, unsigned long long *d_comp_off, uint8_t *d_packed, unsigned long long *totals_out);

static bool sink_on(const pssbam_engine *e) { return e->sink || e->block_sink; }

// both setters: record != NULL sets the record sink, block != NULL the block sink, neither switches `which` off
static int set_sink(pssbam_engine *e, pssbam_record_sink record, pssbam_block_sink block, void *ctx, bool which_block) {
    const char *name = which_block ? "block" : "record";
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (e->tallied || e->cur_feed >= 0 || !e->deferred.empty() || !e->sel_queue.empty())
        return fail(PSSBAM_ESTATE, "the %s sink is set before the first submit (after create or reset)", name);
    if ((record || block) && !(e->cfg.tally_mask & PSSBAM_TALLY_PSS)) return fail(PSSBAM_EINVAL, "the %s sink follows the substitution tally (PSSBAM_TALLY_PSS)", name);
    if (block && e->sink) return fail(PSSBAM_EINVAL, "a record sink is set: the block sink goes instead of it, not beside it");
    if (record && e->block_sink) return fail(PSSBAM_EINVAL, "a block sink is set: the record sink goes instead of it, not beside it");
    const uint64_t before = select_reserve_bytes(e);
    if (which_block) {
        e->block_sink = block;
        e->block_ctx = block ? ctx : nullptr;
    } else {
        e->sink = record;
        e->sink_ctx = record ? ctx : nullptr;
    }
    if (e->feed_mem_budget) {   // worked out already (pssbam_engine_feed_open): the sink's buffers come out of it, or go back
        const uint64_t budget = e->feed_mem_budget + before, after = select_reserve_bytes(e);
        e->feed_mem_budget = budget > after ? budget - after : 1;
    }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_record_sink(pssbam_engine *e, pssbam_record_sink sink, void *ctx) { return set_sink(e, sink, nullptr, ctx, false); }
extern "C" int pssbam_engine_set_block_sink(pssbam_engine *e, pssbam_block_sink sink, void *ctx) { return set_sink(e, nullptr, sink, ctx, true); }

static_assert(PSSBAM_EM_OFF == PSSBAM_END_MASK_OFF && PSSBAM_EM_ALL == PSSBAM_END_MASK_ALL && PSSBAM_EM_DS == PSSBAM_END_MASK_DS &&
              PSSBAM_EM_SS == PSSBAM_END_MASK_SS && PSSBAM_EM_MAX_N == PSSBAM_MAX_END_MASK, "end_mask_kernels.h and pssbam_hip.h name the same modes");

extern "C" int pssbam_engine_set_end_mask(pssbam_engine *e, int32_t mode, uint32_t n5, uint32_t n3) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (e->tallied || e->cur_feed >= 0 || !e->deferred.empty() || !e->sel_queue.empty())
        return fail(PSSBAM_ESTATE, "the end mask is set before the first submit (after create or reset)");
    if (mode < PSSBAM_END_MASK_OFF || mode > PSSBAM_END_MASK_SS) return fail(PSSBAM_EINVAL, "end mask: unknown mode %d (0 off, 1 all, 2 ds, 3 ss)", (int)mode);
    if (n5 > PSSBAM_MAX_END_MASK || n3 > PSSBAM_MAX_END_MASK)
        return fail(PSSBAM_EINVAL, "end mask: the regions are at most %d bases wide, not %u and %u", PSSBAM_MAX_END_MASK, n5, n3);
    if (mode != PSSBAM_END_MASK_OFF && n5 == 0 && n3 == 0) return fail(PSSBAM_EINVAL, "end mask: both regions are empty");
    e->end_mask_mode = (uint32_t)mode;
    e->end_mask_n5 = n5;
    e->end_mask_n3 = n3;
    return PSSBAM_OK;
}

// Moves the buffers in flight along: a buffer whose totals have arrived starts the copy of its data, the oldest buffer
// whose data has arrived is handed to the sink.  wait: until nothing is in flight.
static int select_poll(pssbam_engine *e, bool wait) {
    while (!e->sel_queue.empty()) {
        for (int k : e->sel_queue) {
            SelectBuf &b = e->sel[k];
            if (b.state != SEL_TOTALS) continue;
            if (wait && k == e->sel_queue.front()) HIP_TRY(hipEventSynchronize(b.totals_ev));
            const hipError_t q = hipEventQuery(b.totals_ev);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); break; }   // (the ones behind it are later on the same stream)
            if (q != hipSuccess) return fail(PSSBAM_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
            const uint64_t bytes = b.h_totals[b.deflated ? 2 : 0];
            if (bytes > b.out_cap) return fail(PSSBAM_EHIP, "record selection reports %llu bytes in a buffer of %zu", (unsigned long long)bytes, b.out_cap);
            if (bytes > b.h_cap) {
                if (b.h_data) HIP_TRY(hipHostFree(b.h_data));
                b.h_data = nullptr;
                b.h_cap = (size_t)(bytes + bytes / 4 + (1u << 20));
                HIP_TRY(hipHostMalloc((void **)&b.h_data, b.h_cap, hipHostMallocDefault));
            }
            if (bytes) HIP_TRY(hipMemcpyAsync(b.h_data, b.d_out, bytes, hipMemcpyDeviceToHost, e->sel_stream));
            HIP_TRY(hipEventRecord(b.data_ev, e->sel_stream));
            b.state = SEL_DATA;
        }
        SelectBuf &b = e->sel[e->sel_queue.front()];
        if (b.state != SEL_DATA) return PSSBAM_OK;   // (only without `wait`)
        if (wait) HIP_TRY(hipEventSynchronize(b.data_ev));
        const hipError_t q = hipEventQuery(b.data_ev);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return PSSBAM_OK; }
        if (q != hipSuccess) return fail(PSSBAM_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        b.state = SEL_FREE;
        e->sel_queue.erase(e->sel_queue.begin());
        if (!b.deflated && e->sink && b.h_totals[1] && e->sink(e->sink_ctx, b.h_data, b.h_totals[0], b.h_totals[1]) != 0) {
            e->sink = nullptr;       // never called again; what is still in flight is dropped as it arrives
            e->sink_failed = true;   // reported by select_report, where the engine call can fail without leaving work half queued
            e->block_sink_failed = false;
        }
        if (b.deflated && e->block_sink && b.h_totals[1] &&
            e->block_sink(e->block_ctx, b.h_data, b.h_totals[2], b.h_totals[3], b.h_totals[0], b.h_totals[1]) != 0) {
            e->block_sink = nullptr;
            e->sink_failed = e->block_sink_failed = true;
        }
    }
    return PSSBAM_OK;
}

// The sink's failure becomes the engine call's: only where nothing of the call is queued yet (the top of a submit) or everything
// is through (sync, finish, reset).  A chunk that arrives while a submit is queuing its kernels (launch_select polls too) is
// handed over there, but a failure of the sink waits for the next of these places: the block's tally, its slot's `consumed` event
// and the launches put off for the genome all go on as they would have.
static int select_report(pssbam_engine *e) {
    if (!e->sink_failed) return PSSBAM_OK;
    e->sink_failed = false;
    return fail(PSSBAM_EINVAL, "the %s sink returned non-zero", e->block_sink_failed ? "block" : "record");
}

// the top of every submit: what has arrived goes out, before anything of this call is queued
static int select_entry(pssbam_engine *e, uint64_t nbytes) {
    if (sink_on(e) && nbytes > 0xFFFFFF00ull) return fail(PSSBAM_EINVAL, "record block of %llu bytes is too large for the record sink", (unsigned long long)nbytes);
    if (!e->sel_queue.empty())
        if (const int rc = select_poll(e, false)) return rc;
    return select_report(e);
}

template <class T>
static int select_grow(T **p, size_t *cap, size_t need) {
    if (*cap >= need) return PSSBAM_OK;
    if (*p) HIP_TRY(hipFree(*p));   // (waits for the device: no kernel still reads it)
    *p = nullptr;
    *cap = need + need / 4 + 1024;
    HIP_TRY(hipMalloc((void **)p, *cap * sizeof(T)));
    return PSSBAM_OK;
}

// behind the tally kernels of the block P describes, on the engine's stream
static int launch_select(pssbam_engine *e, const TallyParams &P, uint64_t nbytes) {
    int rc = select_poll(e, false);   // (a sink that fails here is reported by the next select_report: the tally of this block is queued)
    if (rc) return rc;
    const int k = e->sel_next;
    SelectBuf &b = e->sel[k];
    if (b.state != SEL_FREE && (rc = select_poll(e, true))) return rc;   // both buffers in flight: the older one first
    if (!sink_on(e)) return PSSBAM_OK;
    if (!e->sel_stream) HIP_TRY(hipStreamCreateWithFlags(&e->sel_stream, hipStreamNonBlocking));
    if (!b.d_totals) {
        HIP_TRY(hipMalloc((void **)&b.d_totals, 4 * sizeof(unsigned long long)));
        HIP_TRY(hipHostMalloc((void **)&b.h_totals, 4 * sizeof(unsigned long long), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&b.totals_ev, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b.data_ev, hipEventDisableTiming));
    }
    const uint32_t n = P.n_recs, n_tiles = (n + SELECT_SCAN_TILE - 1) / SELECT_SCAN_TILE;
    const bool deflate = e->block_sink != nullptr;
    const size_t n_blocks = (size_t)((nbytes + DFL_PAYLOAD - 1) / DFL_PAYLOAD);   // of the block sink: every record kept
    // every record kept, whole 16-byte stores; the block sink packs its blocks into the same buffer: a stored block is 31 bytes over its payload
    const size_t out_need = (size_t)((nbytes + 15ull) & ~15ull) + 16 + (deflate ? 31 * n_blocks : 0);
    if (b.out_cap < out_need) {
        if (b.d_out) HIP_TRY(hipFree(b.d_out));
        b.d_out = nullptr;
        b.out_cap = out_need + out_need / 8 + 4096;
        HIP_TRY(hipMalloc((void **)&b.d_out, b.out_cap));
    }
    if ((rc = select_grow(&e->d_sel_len, &e->sel_len_cap, (size_t)n + 1))) return rc;
    if ((rc = select_grow(&e->d_sel_sums, &e->sel_sums_cap, (size_t)n_tiles))) return rc;
    if (deflate && e->comp_cap < n_blocks) {
        if (e->d_comp) HIP_TRY(hipFree(e->d_comp));   // (waits for the device: no kernel still reads it)
        if (e->d_comp_len) HIP_TRY(hipFree(e->d_comp_len));
        if (e->d_comp_off) HIP_TRY(hipFree(e->d_comp_off));
        e->d_comp = nullptr;
        e->d_comp_len = nullptr;
        e->d_comp_off = nullptr;
        e->comp_cap = 0;
        const size_t cap_blocks = n_blocks + n_blocks / 8 + 16;
        HIP_TRY(hipMalloc((void **)&e->d_comp, cap_blocks * DFL_SLOT));
        HIP_TRY(hipMalloc((void **)&e->d_comp_len, cap_blocks * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&e->d_comp_off, cap_blocks * sizeof(unsigned long long)));
        e->comp_cap = cap_blocks;
    }
    const uint32_t cap = (uint32_t)e->n_cu * 8u;
    const uint32_t g_mark = (uint32_t)std::min<uint64_t>(((uint64_t)n + 1 + 255) / 256, cap), g_tiles = std::min(n_tiles, cap);
    const uint64_t pieces = (nbytes / 16 + 1 + SELECT_GATHER_THREADS * SELECT_GATHER_CHUNKS - 1) / (SELECT_GATHER_THREADS * SELECT_GATHER_CHUNKS);
    const uint32_t g_gather = (uint32_t)std::min<uint64_t>(pieces, cap);
    hipLaunchKernelGGL(select_mark, dim3(g_mark), dim3(256), 0, e->stream, P, e->d_sel_len);
    hipLaunchKernelGGL(select_tile_sums, dim3(g_tiles), dim3(SELECT_SCAN_THREADS), 0, e->stream, (const uint32_t *)e->d_sel_len, n, e->d_sel_sums);
    hipLaunchKernelGGL(select_scan_sums, dim3(1), dim3(SELECT_SUMS_ROUND), 0, e->stream, e->d_sel_sums, n_tiles, b.d_totals);
    hipLaunchKernelGGL(select_scan_tiles, dim3(g_tiles), dim3(SELECT_SCAN_THREADS), 0, e->stream, e->d_sel_len, n, (const uint2 *)e->d_sel_sums,
                       (const unsigned long long *)b.d_totals);
    hipLaunchKernelGGL(select_gather, dim3(g_gather), dim3(SELECT_GATHER_THREADS), 0, e->stream, P.recs, P.offs, (const uint32_t *)e->d_sel_len, n,
                       (const unsigned long long *)b.d_totals, b.d_out);
    const bool mask = e->end_mask_mode != PSSBAM_END_MASK_OFF;
    if (mask)   // in the output copy, in front of the deflate and of the copy to the host (started behind totals_ev)
        hipLaunchKernelGGL(select_mask_ends, dim3(std::max(1u, std::min((n + 255u) / 256u, cap))), dim3(256), 0, e->stream, b.d_out,
                           (const uint32_t *)e->d_sel_len, n, nbytes, e->end_mask_mode, e->end_mask_n5, e->end_mask_n3);
    HIP_TRY(hipGetLastError());
    if (deflate && (rc = launch_deflate(e->stream, b.d_out, nbytes, b.d_totals, e->d_comp, e->d_comp_len, e->d_comp_off, b.d_out, b.d_totals + 2))) return rc;
    b.deflated = deflate;
    HIP_TRY(hipMemcpyAsync(b.h_totals, b.d_totals, (deflate ? 4 : 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipEventRecord(b.totals_ev, e->stream));
    b.state = SEL_TOTALS;
    e->sel_queue.push_back(k);
    e->sel_next ^= 1;
    e->sel_launches += (deflate ? 8 : 5) + (mask ? 1 : 0);
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// duplicate flagging: insert + resolve in front of a block's tally kernels (dedup_kernels.h)
// --------------------------------------------------------------------------------------
static constexpr uint64_t DEDUP_DEFAULT_SLOTS = 1ull << 20, DEDUP_MAX_SLOTS = 1ull << 31;   // (a slot index fits slot_of[]'s 32 bits beside DEDUP_NO_SLOT)

static uint64_t dedup_first_slots(const pssbam_engine *e) {
    uint64_t cap = 16;
    const uint64_t want = e->dedup_initial ? e->dedup_initial : DEDUP_DEFAULT_SLOTS;
    while (cap < want) cap <<= 1;
    return cap;
}

static uint64_t dedup_reserve_bytes(const pssbam_engine *e);   // (bgzf_api.h: what the table and slot_of[] take from the feed's memory budget)

static uint32_t dedup_grid(const pssbam_engine *e, uint64_t lanes) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 255) / 256, (uint64_t)e->n_cu * 8));
}

// the state word that has arrived, if one has: the occupied count the growth rule starts from, and the table-full error
static int dedup_poll(pssbam_engine *e, bool wait) {
    for (size_t i = 0; i < e->dedup_old.size();) {   // tables the stream has passed
        const hipError_t q = wait ? hipEventSynchronize(e->dedup_old[i].second) : hipEventQuery(e->dedup_old[i].second);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); i++; continue; }
        if (q != hipSuccess) return fail(PSSBAM_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        HIP_TRY(hipFree(e->dedup_old[i].first));
        HIP_TRY(hipEventDestroy(e->dedup_old[i].second));
        e->dedup_old.erase(e->dedup_old.begin() + (long)i);
    }
    if (!e->dedup_reading) return PSSBAM_OK;
    const hipError_t q = wait ? hipEventSynchronize(e->dedup_ev) : hipEventQuery(e->dedup_ev);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return PSSBAM_OK; }
    if (q != hipSuccess) return fail(PSSBAM_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
    e->dedup_reading = false;
    const unsigned long long st = *e->h_dedup_state;
    if (st & DEDUP_FULL) return fail(PSSBAM_ENOMEM, "the duplicate table ran full (%llu slots): records went unflagged", (unsigned long long)e->dedup_cap);
    e->dedup_known = st;
    e->dedup_known_at = e->dedup_reading_at;
    return PSSBAM_OK;
}

// an empty table of `cap` slots; with an old one, its keys go over first
static int dedup_table(pssbam_engine *e, uint64_t cap) {
    if (cap > DEDUP_MAX_SLOTS) return fail(PSSBAM_ENOMEM, "the duplicate table would pass %llu slots", (unsigned long long)DEDUP_MAX_SLOTS);
    DedupSlot *d_new = nullptr;
    if (hipMalloc((void **)&d_new, cap * sizeof(DedupSlot)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PSSBAM_ENOMEM, "a duplicate table of %llu slots (%llu bytes) does not fit the device", (unsigned long long)cap,
                    (unsigned long long)(cap * sizeof(DedupSlot)));
    }
    hipLaunchKernelGGL(dedup_clear, dim3(dedup_grid(e, cap)), dim3(256), 0, e->stream, d_new, cap);
    e->dedup_launches++;
    if (e->d_dedup) {
        if (e->dedup_submitted) {   // (a table nothing was inserted into has nothing to carry over)
            hipLaunchKernelGGL(dedup_rehash, dim3(dedup_grid(e, e->dedup_cap)), dim3(256), 0, e->stream, (const DedupSlot *)e->d_dedup, e->dedup_cap, d_new,
                               (uint32_t)(cap - 1), e->d_dedup_state);
            e->dedup_launches++;
        }
        hipEvent_t passed = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&passed, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(passed, e->stream));
        e->dedup_old.emplace_back((void *)e->d_dedup, passed);
    }
    HIP_TRY(hipGetLastError());
    e->d_dedup = d_new;
    e->dedup_cap = cap;
    return PSSBAM_OK;
}

// In front of the tally kernels of the block P describes, on the engine's stream: the block's duplicates get FLAG bit 0x400 in the
// device copy of the records.  Before the insert the table has at least twice as many slots as it can hold keys afterwards: the
// occupied slots as last known plus every record submitted since that reading, this block's included (the host's bound).
static int launch_dedup(pssbam_engine *e, const TallyParams &P) {
    int rc = dedup_poll(e, false);
    if (rc) return rc;
    if (!e->d_dedup_state) {
        HIP_TRY(hipMalloc((void **)&e->d_dedup_state, sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(e->d_dedup_state, 0, sizeof(unsigned long long), e->stream));
        HIP_TRY(hipHostMalloc((void **)&e->h_dedup_state, sizeof(unsigned long long), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->dedup_ev, hipEventDisableTiming));
    }
    const uint64_t need = 2 * (e->dedup_known + (e->dedup_submitted - e->dedup_known_at) + P.n_recs);
    uint64_t cap = e->dedup_cap ? e->dedup_cap : dedup_first_slots(e);
    while (cap < need) cap <<= 1;
    if (cap != e->dedup_cap && (rc = dedup_table(e, cap))) return rc;
    if ((rc = select_grow(&e->d_dedup_slot, &e->dedup_slot_cap, (size_t)P.n_recs))) return rc;
    const uint32_t grid = dedup_grid(e, P.n_recs), seq = e->dedup_seq++;
    const bool groups = e->planes == PLANES_RG;
    hipLaunchKernelGGL(dedup_insert, dim3(grid), dim3(256), 0, e->stream, P, plane_params(e), groups ? 1u : 0u, e->d_dedup, (uint32_t)(e->dedup_cap - 1), seq,
                       e->d_dedup_slot, e->d_dedup_state);
    hipLaunchKernelGGL(dedup_resolve, dim3(grid), dim3(256), 0, e->stream, const_cast<uint8_t *>(P.recs), P.offs, P.n_recs, (const DedupSlot *)e->d_dedup, seq,
                       (const uint32_t *)e->d_dedup_slot);
    HIP_TRY(hipGetLastError());
    e->dedup_launches += 2;
    e->dedup_submitted += P.n_recs;
    if (!e->dedup_reading) {
        HIP_TRY(hipMemcpyAsync(e->h_dedup_state, e->d_dedup_state, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipEventRecord(e->dedup_ev, e->stream));
        e->dedup_reading = true;
        e->dedup_reading_at = e->dedup_submitted;
    }
    return PSSBAM_OK;
}

// d_n_recs != NULL: the record count lives in device memory (blocks indexed on the device); n_records
// is then only an upper bound for the launch geometry, and the prefix sample is taken sample_off
// bytes into the block.
static int launch_tally(pssbam_engine *e, const uint8_t *d_recs, uint64_t nbytes, const uint32_t *d_offs,
                        uint32_t n_records, const uint8_t *host_sample, uint64_t host_sample_bytes,
                        const uint32_t *d_n_recs = nullptr, uint64_t sample_off = 0, const uint32_t *host_offsets = nullptr) {
    if (!n_records) return PSSBAM_OK;
    e->tallied = true;
    const pssbam_config &c = e->cfg;
    TallyParams P{};
    P.recs = d_recs;
    P.offs = d_offs;
    P.n_recs = n_records;
    P.n_recs_dev = d_n_recs;
    P.recs_bytes = nbytes;
    P.tally_mask = c.tally_mask;
    P.genome = e->d_genome;
    P.genome4 = e->d_genome4;
    P.acgt_ctx = e->acgt_ctx;
    P.ref_info = e->d_ref_info;
    P.n_ref = e->n_ref;
    const bool do_pss = (c.tally_mask & PSSBAM_TALLY_PSS) != 0, do_kmer = (c.tally_mask & PSSBAM_TALLY_KMER) != 0;
    if (do_pss) {
        P.N = c.pss.region_len;
        P.pss_min_mq = (uint32_t)c.pss.min_mq;
        P.pss_len_never = c.pss.min_read_len > 0xFFFFFFFFull ? 1u : 0u;
        P.pss_min_len = (uint32_t)std::min<uint64_t>(c.pss.min_read_len, 0xFFFFFFFFull);
        P.pss_max_len = (uint32_t)std::min<uint64_t>(c.pss.max_read_len, 0xFFFFFFFFull);
        P.pss_merged_only = c.pss.merged_only ? 1u : 0u;
        ctx_mask(e->up_ctx.c_str(), P.up_mask);
        ctx_mask(e->down_ctx.c_str(), P.down_mask);
    }
    if (do_kmer) {
        P.K = c.kmer.klen;
        P.fk_min_mq = (uint32_t)c.kmer.min_mq;
        P.fk_len_never = c.kmer.min_read_len > 0xFFFFFFFFull ? 1u : 0u;
        P.fk_min_len = (uint32_t)std::min<uint64_t>(c.kmer.min_read_len, 0xFFFFFFFFull);
        P.fk_max_len = (uint32_t)std::min<uint64_t>(c.kmer.max_read_len, 0xFFFFFFFFull);
        P.fk_merged_only = c.kmer.merged_only ? 1u : 0u;
    }
    P.rg = e->has_rg ? e->d_rg : nullptr;
    P.rg_len = (uint32_t)e->rg.size();
    P.counters = e->d_counters;
    P.off_rev = e->off_rev;
    P.off_k5 = e->off_k5;
    P.off_k3 = e->off_k3;
    P.off_stats = e->off_stats;
    P.min_bq = do_pss ? e->min_bq : 0u;
    const bool maskq = P.min_bq > 0;   // -Q: the MASKQ instantiations of the tiled kernels; min_bq == 0 launches what it always did
    const bool regions = e->has_regions;   // -T: the REGIONS instantiations; without regions the engine launches what it always did
    // -H, -X, -E, -I, -n / -N, -W, -P, -y / -Y: the instantiations with the mode's arm; an engine without a mode launches what it always did
    const TallyArm arm = tally_arm(e);
    if (arm == ARM_HIST) {
        P.hist_max = e->hist_max;
        P.off_hist = e->off_groups;
    } else if (arm == ARM_SITE) {
        P.off_site = e->off_groups;
    } else if (arm == ARM_END) {
        P.end_depth = e->end_depth;
        P.end_cell5 = e->end_cell5;
        P.end_cell3 = e->end_cell3;
        P.off_end = e->off_groups;
    } else if (arm == ARM_GAPPED) {
        P.gapped = 1u;
    } else if (arm == ARM_MISM) {
        P.mism_limit = e->mism_max >= 0 ? (uint32_t)e->mism_max + 1u : 0u;
        P.mism_hist = e->mism_hist;
        P.mism_tv = e->mism_tv ? 1u : 0u;
        P.off_mism = e->mism_hist ? e->off_groups : 0u;
    } else if (arm == ARM_INTERIOR) {
        P.interior = (uint32_t)e->interior_margin + 1u;
        P.off_interior = e->off_groups;
    } else if (arm == ARM_COMP) {
        P.composition = e->composition;
        P.off_composition = e->off_groups;
    } else if (arm == ARM_SCORE) {
        P.score_w = e->d_score_w;
        P.score_nd = e->score_nd;
        P.score_nq = e->score_nq;
        P.score_filter = e->score_filter ? 1u : 0u;
        P.score_min = e->score_min;
        P.score_half = e->score_half;
        P.score_shift = e->score_shift;
        P.off_score = e->score_half ? e->off_groups : 0u;
    }
    if (regions) {
        P.region_info = e->d_region_info;
        P.region_grid = e->d_region_grid;
        P.region_iv = e->d_region_iv;
        P.region_shift = e->region_shift;
    }
    PlaneParams G = plane_params(e);

    int kernel = c.kernel;
    if (d_n_recs && kernel == PSSBAM_KERNEL_SIMPLE) return fail(PSSBAM_EINVAL, "device-indexed blocks need the tiled kernels");
    // the tiled kernel covers 32 table rows per pass over the block (measured on C3: N=30 18 G
    // reads/s, N=62 9.3 G, N=100 4.8 G; the generic kernel: 0.77 / 0.37 / 0.23 G and falling with
    // N), so it is the automatic choice for every N; the generic kernel is the cross-check
    const uint32_t n_passes = do_pss ? (e->rows + TILED_ROWS - 1) / TILED_ROWS : 1u;
    if (kernel == PSSBAM_KERNEL_AUTO) kernel = PSSBAM_KERNEL_TILED;

    if (e->genome_wait_pending) {   // the upload runs on its own stream
        HIP_TRY(hipStreamWaitEvent(e->stream, e->genome_ready, 0));
        e->genome_wait_pending = false;
    }
    // duplicate flagging: in front of the tally kernels and of the opening event -- the time and the launch count stay the tally's
    if (e->dedup)
        if (const int rc = launch_dedup(e, P)) return rc;
    hipEvent_t ev0 = take_event(e), ev1 = take_event(e);
    if (!ev0 || !ev1) return fail(PSSBAM_EHIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(ev0, e->stream));

    if (kernel == PSSBAM_KERNEL_SIMPLE) {
        const uint32_t tab_bytes = do_pss ? 2u * e->rows * 16u * 4u : 0u;
        const bool lds_tab = do_pss && tab_bytes <= 60u * 1024u;
        uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_records + 255) / 256, (uint64_t)e->n_cu * 8);
        if (e->env_simple_blocks > 0) blocks = (uint32_t)e->env_simple_blocks;
        if (e->planes == PLANES_EACH)   // -A: straight into every reference's plane
            hipLaunchKernelGGL(tally_simple_planes<PLANES_EACH>, dim3(blocks), dim3(256), 0, e->stream, P, G);
        else if (e->planes != PLANES_NONE)
            with_planes(e->planes, [&](auto SEL) {
                if (do_pss) hipLaunchKernelGGL(tally_simple_planes<SEL()>, dim3(blocks), dim3(256), 0, e->stream, P, G);
                else if constexpr (SEL() == PLANES_HASH) return no_kernel();   // (replicates split the substitution tables only: set_replicates)
                else hipLaunchKernelGGL(tally_simple_kmer_planes<SEL()>, dim3(blocks), dim3(256), 0, e->stream, P, G);
                return PSSBAM_OK;
            });
        else if (lds_tab) hipLaunchKernelGGL(tally_simple<true>, dim3(blocks), dim3(256), tab_bytes, e->stream, P);
        else hipLaunchKernelGGL(tally_simple<false>, dim3(blocks), dim3(256), 0, e->stream, P);
    } else {
        // how much of each record goes through LDS: sampled from the block itself (host copy at
        // hand for submit(); for device-resident blocks a one-off 64 KiB read-back, remembered
        // while the mean record size stays put)
        const uint64_t avg = std::max<uint64_t>(40, nbytes / n_records);
        uint32_t pieces;
        if (host_sample) {
            // three regions of the block (start, middle, end: 1400 records each), found through the
            // caller's offset index -- a block whose later records are longer than its first ones must
            // not silently fall onto the one-lane path (stats.slow_path)
            uint64_t need = sample_prefix_need(host_sample, host_sample_bytes, whole_records(e), 1400);
            if (host_offsets && n_records > 4200u) {
                const uint32_t mid = host_offsets[n_records / 2], late = host_offsets[n_records - 1400u];
                need = std::max(need, sample_prefix_need(host_sample + mid, host_sample_bytes - mid, whole_records(e), 1400));
                need = std::max(need, sample_prefix_need(host_sample + late, host_sample_bytes - late, whole_records(e), 1400));
            }
            pieces = pieces_for(need);
        } else {
            if (!e->dev_pieces || (!d_n_recs && (avg * 8 < e->dev_pieces_avg * 7 || avg * 7 > e->dev_pieces_avg * 8))) {
                sample_off = std::min<uint64_t>(sample_off, nbytes);
                std::vector<uint8_t> head((size_t)std::min<uint64_t>(nbytes - sample_off, 1024 * 1024));
                HIP_TRY(hipMemcpyAsync(head.data(), d_recs + sample_off, head.size(), hipMemcpyDeviceToHost, e->stream));
                HIP_TRY(hipStreamSynchronize(e->stream));
                uint64_t need = sample_prefix_need(head.data(), head.size(), whole_records(e));
                if (!d_n_recs && n_records > 8192u) {   // device-resident block with a known count: its middle and end too
                    uint32_t at[2] = {0, 0};
                    HIP_TRY(hipMemcpyAsync(&at[0], d_offs + n_records / 2, 4, hipMemcpyDeviceToHost, e->stream));
                    HIP_TRY(hipMemcpyAsync(&at[1], d_offs + (n_records - 2048u), 4, hipMemcpyDeviceToHost, e->stream));
                    HIP_TRY(hipStreamSynchronize(e->stream));
                    for (int k = 0; k < 2; k++) {
                        if ((uint64_t)at[k] >= nbytes) continue;
                        head.resize((size_t)std::min<uint64_t>(nbytes - at[k], 512 * 1024));
                        HIP_TRY(hipMemcpyAsync(head.data(), d_recs + at[k], head.size(), hipMemcpyDeviceToHost, e->stream));
                        HIP_TRY(hipStreamSynchronize(e->stream));
                        need = std::max(need, sample_prefix_need(head.data(), head.size(), whole_records(e), 2048));
                    }
                }
                e->dev_pieces = pieces_for(need);
                e->dev_pieces_avg = avg;
            }
            pieces = e->dev_pieces;
        }
        if (e->env_pieces > 0) pieces = (uint32_t)std::min(std::max(e->env_pieces, 4), 64);
        uint32_t T = TILED_MAX_T;
        if (e->env_tile_reads > 0) T = std::min<uint32_t>(TILED_MAX_T, (uint32_t)(e->env_tile_reads + 15) / 16 * 16);
        P.reads_per_tile = T;
        P.prefix_pieces = pieces;
        P.xcd_map = (uint32_t)env_int("PSSBAM_XCD_MAP");
        P.ablate = (uint32_t)env_int("PSSBAM_ABLATE");  // profiling aid (tools/ablate.sh): switches kernel phases off
        if (P.ablate && !e->warned_ablate) {
            fprintf(stderr, "[pssbam] PSSBAM_ABLATE=%u: kernel phases are switched off, the tables are WRONG (profiling only)\n", P.ablate);
            e->warned_ablate = true;
        }
        const bool kmer_lds = do_kmer && c.kmer.klen <= KMER_LDS_MAX_K;
        const uint32_t n_tiles = (n_records + T - 1) / T;
        const uint32_t lds = tiled_lds_bytes(T, pieces);
        int rc = PSSBAM_OK;
        P.row_base = 0;
        if (e->planes == PLANES_EACH) {
            // -A: one launch per 32-row pass whatever the number of references.  A workgroup holds `slots` planes (4 KiB each)
            // and the trash plane behind the staging buffer; the planes leave LDS straight into the counter block, so a
            // workgroup's scratch slot is the status deltas alone and reduce_partials_grouped walks nothing else.
            uint32_t slots = e->env_contig_slots > 0 ? (uint32_t)e->env_contig_slots : EACH_DEFAULT_SLOTS;
            const uint32_t fit = lds + 2u * GROUP_PLANE_WORDS * 4u <= GROUPED_LDS_BUDGET ? (GROUPED_LDS_BUDGET - lds) / (GROUP_PLANE_WORDS * 4u) - 1u : 1u;
            slots = std::max(1u, std::min({slots, fit, EACH_MAX_SLOTS, G.n_groups}));
            G.plane0 = 0;
            G.each_evict = e->contig_evict ? 1u : 0u;
            G.n_slots = slots;
            G.scratch_words = GROUP_SCRATCH_DELTA;
            for (uint32_t pass = 0; pass < n_passes && rc == PSSBAM_OK; pass++) {
                P.row_base = pass * TILED_ROWS;
                rc = with_flags([&](auto LATER, auto MASKQ, auto REGIONS) {
                    return launch_with_reduce(e, tally_tiled_planes<PLANES_EACH, LATER(), MASKQ(), REGIONS()>, reduce_partials_grouped, G.scratch_words,
                                              tiled_grouped_lds_bytes(T, pieces, slots), n_tiles, P, std::tie(G));
                }, pass > 0, maskq, regions);
            }
        } else if (e->planes != PLANES_NONE) {
            // -G / -S / -C / -J: every (32-row pass, plane pass) pair is one launch over the block.  A plane pass holds as many
            // planes as fit the LDS beside the staging buffer, plus a trash plane; more planes take more passes, each
            // re-reading the records.  Substitution planes are 4 KiB each (8 = 32 KiB always fit: one pass for up to 7 groups
            // or sets, or 6 bins -- plane 0 of -S stays empty but keeps its slot).  K-mer planes (one row pass) are
            // 2 * 4^k-word histograms at k <= KMER_LDS_MAX_K -- 2 KiB each at k = 4, so 64 bins and plane 0 are one pass;
            // larger k: global atomics, no plane in LDS, one pass whatever the count.
            const uint32_t n_planes = G.n_groups + 1u;
            const uint32_t plane_bytes = do_pss ? GROUP_PLANE_WORDS * 4u : kmer_lds ? 2u * (1u << (2 * c.kmer.klen)) * 4u : 0u;
            const uint32_t budget = do_pss ? GROUPED_LDS_BUDGET : KMER_PLANES_LDS_BUDGET;
            uint32_t per_pass = n_planes;
            if (plane_bytes) {
                const uint32_t fit = lds + 2u * plane_bytes <= budget ? (budget - lds) / plane_bytes - 1u : 1u;
                per_pass = std::min(n_planes, fit);
                if (e->env_group_slots > 0) per_pass = std::min(per_pass, (uint32_t)e->env_group_slots);
            }
            for (uint32_t pass = 0; pass < n_passes && rc == PSSBAM_OK; pass++) {
                P.row_base = pass * TILED_ROWS;
                for (uint32_t plane0 = 0; plane0 < n_planes && rc == PSSBAM_OK; plane0 += per_pass) {
                    G.plane0 = plane0;
                    G.n_slots = std::min(per_pass, n_planes - plane0);
                    G.scratch_words = GROUP_SCRATCH_DELTA + G.n_slots * (plane_bytes / 4u);
                    rc = with_planes(e->planes, [&](auto SEL) {
                        if (do_pss)
                            return with_flags([&](auto LATER, auto MASKQ, auto REGIONS) {
                                return launch_with_reduce(e, tally_tiled_planes<SEL(), LATER(), MASKQ(), REGIONS()>, reduce_partials_grouped, G.scratch_words,
                                                          tiled_grouped_lds_bytes(T, pieces, G.n_slots), n_tiles, P, std::tie(G));
                            }, pass > 0, maskq, regions);
                        if constexpr (SEL() == PLANES_HASH) return no_kernel();   // (replicates split the substitution tables only: set_replicates)
                        else
                        return with_flags([&](auto LDS_KMER, auto REGIONS) {
                            return launch_with_reduce(e, tally_tiled_kmer_planes<SEL(), LDS_KMER(), REGIONS()>, reduce_partials_kmer_planes, G.scratch_words,
                                                      tiled_kmer_planes_lds_bytes(T, pieces, G.n_slots, c.kmer.klen, LDS_KMER()), n_tiles, P, std::tie(G),
                                                      (uint32_t)LDS_KMER());
                        }, kmer_lds, regions);
                    });
                }
            }
        } else if (do_pss && e->rows <= COMPACT_MAX_ROWS && e->use_compact && !e->has_rg && !maskq && !regions && arm == ARM_NONE) {
            // -r N <= 16 (2 context rows + 16 positions): the short-window variant, one pass (it stages prefixes only
            // and has no QUAL path: -R and -Q go to tally_tiled; so do -T and every mode with an arm, which only tally_tiled carries)
            if (!do_kmer && getenv("PSSBAM_COMPACT_DECODE_TWICE"))   // diagnostics: what the shared header decode costs
                rc = launch_with_reduce(e, tally_compact_decode_twice, reduce_partials<false>, SCRATCH_WORDS, lds, n_tiles, P, std::tuple<>(), 0u);
            else
                rc = with_flags([&](auto DO_KMER, auto LDS_KMER, auto PLAN_ONCE) -> int {
                    if constexpr (DO_KMER() || !LDS_KMER())
                        return launch_with_reduce(e, tally_compact<DO_KMER(), LDS_KMER(), PLAN_ONCE()>, reduce_partials<false>, SCRATCH_WORDS, lds, n_tiles, P,
                                                  std::tuple<>(), (uint32_t)LDS_KMER());
                    else
                        return no_kernel();
                }, do_kmer, kmer_lds, e->compact_plan_once);
        } else {
            // tally_tiled, 32 table rows per pass over the block.  Pass 0 has the status counters, the k-mer tally and what its
            // arm keeps in LDS behind the staging buffer; rows 32.. of a large -r are further passes, substitution rows only,
            // that count nothing of these again.  The arms but -H, -X and -I are one pass: -r <= 30.
            uint32_t lds0 = lds;
            switch (arm) {
            case ARM_HIST:   // the LDS part of [hf | hr], at most HIST_LDS_MAX_BINS bins each: 8 KiB
                P.hist_lds_bins = std::min(e->hist_max + 2u, HIST_LDS_MAX_BINS);
                if (e->env_hist_lds_bins >= 0) P.hist_lds_bins = std::min(P.hist_lds_bins, (uint32_t)e->env_hist_lds_bins);
                lds0 += hist_lds_bytes(P.hist_lds_bins);
                break;
            case ARM_END: lds0 += end_lds_bytes(e->rows); break;   // the conditional tables and reads[4]
            case ARM_MISM: lds0 += e->mism_hist ? 2u * (e->mism_hist + 2u) * 4u : 0u; break;   // -N: [mf | mr], at most 2 KiB
            case ARM_INTERIOR: lds0 += INTERIOR_WORDS * 4u; break;   // [table | reads]
            case ARM_COMP: lds0 += 20u * e->composition * 4u; break;   // [c5 | c3], at most 2400 bytes
            case ARM_SCORE: lds0 += 4u * e->score_half * 4u; break;   // -Y: [sf | sr], at most 2 KiB (never tally_compact, which has no QUAL path)
            default: break;   // (-X: a static object of the kernel; -I: nothing)
            }
            const TallyArm later_arm = arm == ARM_SITE || arm == ARM_GAPPED ? arm : ARM_NONE;   // the two arms that work on every row
            for (uint32_t pass = 0; pass < n_passes && rc == PSSBAM_OK; pass++) {
                P.row_base = pass * TILED_ROWS;
                rc = pass == 0 ? launch_tiled(e, P, do_pss, do_kmer, kmer_lds, false, maskq, regions, arm, lds0, n_tiles)
                               : launch_tiled(e, P, true, false, false, true, maskq, regions, later_arm, lds, n_tiles);
            }
        }
        if (rc != PSSBAM_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, e->stream));
    e->launch_events.emplace_back(ev0, ev1);
    if (e->launch_events.size() > 4096)
        if (const int rc = resolve_launch_events(e)) return rc;
    // depth of coverage: the kept records' two differences each, behind the tally and its closing event (time and launch count stay
    // the tally's) and, like the sink's kernels, in front of whatever frees the block's buffers
    if (e->coverage) {
        if (!e->d_cov) return fail(PSSBAM_ESTATE, "coverage is on but the genome's array is missing");
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n_records + 255) / 256, (uint64_t)e->n_cu * 8));
        hipLaunchKernelGGL(coverage_add, dim3(grid), dim3(256), 0, e->stream, P, e->d_cov, e->cov_len);
        HIP_TRY(hipGetLastError());
        e->cov_totals_valid = false;
    }
    // allele counts at the listed sites: behind the tally like the coverage's kernel; nothing is launched while no site is resolved
    if (e->has_sites && e->d_site_idx) {
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n_records + 255) / 256, (uint64_t)e->n_cu * 8));
        hipLaunchKernelGGL(allele_add, dim3(grid), dim3(256), 0, e->stream, P, (const uint64_t *)e->d_site_idx, (uint32_t)e->site_idx.size(),
                           (const uint32_t *)e->d_site_grid, e->site_cells, e->site_shift, e->site_trim, e->d_site_counts);
        HIP_TRY(hipGetLastError());
    }
    // the record sink: the kept records of this block, behind its tally and in front of whatever frees the block's buffers
    if (sink_on(e)) return launch_select(e, P, nbytes);
    return PSSBAM_OK;
}

// A caller that will only hand over device-resident or compressed blocks can show the engine a few
// host-side records first: the tiled kernels' staged prefix is then sized from them instead of from a
// read-back of the first block (which has to wait for that block to be inflated).
extern "C" int pssbam_engine_hint_records(pssbam_engine *e, const void *records, uint64_t nbytes) {
    if (!e || (!records && nbytes)) return fail(PSSBAM_EINVAL, "null argument");
    if (nbytes < 36) return PSSBAM_OK;
    e->dev_pieces = pieces_for(sample_prefix_need((const uint8_t *)records, nbytes, whole_records(e), 1 << 16));
    e->dev_pieces_avg = 40;
    return PSSBAM_OK;
}

static int check_ready(pssbam_engine *e) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->d_genome) return fail(PSSBAM_ESTATE, "set_genome has not been called");
    if (!e->have_refs) return fail(PSSBAM_ESTATE, "set_references has not been called");
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_submit_device(pssbam_engine *e, const void *d_records, uint64_t nbytes,
                                           const uint32_t *d_offsets, uint32_t n_records) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (n_records && (!d_records || !d_offsets)) return fail(PSSBAM_EINVAL, "null buffer");
    if (nbytes >= (1ull << 32)) return fail(PSSBAM_EINVAL, "record block must be < 4 GiB (got %llu)", (unsigned long long)nbytes);
    if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_offsets & 3u))
        return fail(PSSBAM_EINVAL, "d_records must be 16-byte aligned, d_offsets 4-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = select_entry(e, nbytes))) return rc;
    return launch_tally(e, (const uint8_t *)d_records, nbytes, d_offsets, n_records, nullptr, 0);
}

// books the H2D duration of a slot whose copy is known to be complete
static void book_copy_time(pssbam_engine *e, Slot &s) {
    if (!s.timed) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.copy_begin, s.copied) == hipSuccess) e->h2d_ms += ms;
    s.timed = false;
}

extern "C" int pssbam_engine_submit_async(pssbam_engine *e, const void *records, uint64_t nbytes, const uint32_t *offsets,
                                          uint32_t n_records, uint64_t *ticket) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (ticket) *ticket = 0;
    if (sink_on(e) || e->sink_failed || !e->sel_queue.empty()) {   // the record sink: an empty submit is a poll, too
        HIP_TRY(hipSetDevice(e->device));
        if ((rc = select_entry(e, n_records ? nbytes : 0))) return rc;
    }
    if (!n_records) return PSSBAM_OK;
    if (!records || !offsets) return fail(PSSBAM_EINVAL, "null buffer");
    if (nbytes >= (1ull << 32)) return fail(PSSBAM_EINVAL, "record block must be < 4 GiB (got %llu)", (unsigned long long)nbytes);
    if (offsets[n_records] != nbytes) return fail(PSSBAM_EFORMAT, "offsets[n_records] must equal nbytes");
    HIP_TRY(hipSetDevice(e->device));
    Slot &s = e->slots[e->next_slot];
    e->next_slot ^= 1;
    if (s.busy) HIP_TRY(hipEventSynchronize(s.consumed));  // the kernel that read this slot is done (so is its copy)
    s.busy = false;
    book_copy_time(e, s);
    if (s.recs_cap < nbytes + 64) {
        if (s.d_recs) HIP_TRY(hipFree(s.d_recs));
        s.d_recs = nullptr;
        s.recs_cap = (size_t)(nbytes + nbytes / 4 + 4096);
        HIP_TRY(hipMalloc(&s.d_recs, s.recs_cap));
    }
    if (s.offs_cap < (size_t)n_records + 1) {
        if (s.d_offs) HIP_TRY(hipFree(s.d_offs));
        s.d_offs = nullptr;
        s.offs_cap = (size_t)n_records + n_records / 4 + 1024;
        HIP_TRY(hipMalloc(&s.d_offs, s.offs_cap * sizeof(uint32_t)));
    }
    // H2D on the copy stream so it overlaps the previous block's kernel
    // large blocks go over two copy streams (two DMA engines): one stream alone does not fill
    // the PCIe link
    late_streams(e, true);   // (this path copies on a stream of its own from the first block on)
    if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    const uint64_t half = (nbytes >= (64ull << 20) && e->copy_stream2 && !getenv("PSSBAM_ONE_COPY_STREAM")) ? (nbytes / 2) & ~4095ull : 0;
    HIP_TRY(hipEventRecord(s.copy_begin, e->copy_stream));
    if (half) {
        HIP_TRY(hipStreamWaitEvent(e->copy_stream2, s.copy_begin, 0));
        HIP_TRY(hipMemcpyAsync(s.d_recs + half, (const uint8_t *)records + half, nbytes - half, hipMemcpyHostToDevice, e->copy_stream2));
        HIP_TRY(hipEventRecord(e->copied2, e->copy_stream2));
    }
    HIP_TRY(hipMemcpyAsync(s.d_recs, records, half ? half : nbytes, hipMemcpyHostToDevice, e->copy_stream));
    HIP_TRY(hipMemcpyAsync(s.d_offs, offsets, ((size_t)n_records + 1) * sizeof(uint32_t), hipMemcpyHostToDevice,
                           e->copy_stream));
    if (half) HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->copied2, 0));  // `copied` then covers both halves
    HIP_TRY(hipEventRecord(s.copied, e->copy_stream));
    s.timed = true;
    e->h2d_bytes += nbytes + ((uint64_t)n_records + 1) * sizeof(uint32_t);
    HIP_TRY(hipStreamWaitEvent(e->stream, s.copied, 0));
    rc = launch_tally(e, s.d_recs, nbytes, s.d_offs, n_records, (const uint8_t *)records, nbytes, nullptr, 0, offsets);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.consumed, e->stream));
    s.busy = true;
    s.ticket = ++e->ticket_seq;
    if (ticket) *ticket = s.ticket;
    return PSSBAM_OK;
}

// 1 = the copy of that submit has completed (its host buffers are free), 0 = still in flight
extern "C" int pssbam_engine_copy_done(pssbam_engine *e, uint64_t ticket) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!ticket) return 1;
    for (Slot &s : e->slots)
        if (s.ticket == ticket) {
            HIP_TRY(hipSetDevice(e->device));
            const hipError_t q = hipEventQuery(s.copied);
            if (q == hipSuccess) return 1;
            if (q == hipErrorNotReady) return 0;
            return fail(PSSBAM_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        }
    return 1;  // the slot has been reused since: that submit waited for the kernel behind this copy
}

extern "C" int pssbam_engine_wait_copied(pssbam_engine *e, uint64_t ticket) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!ticket) return PSSBAM_OK;
    for (Slot &s : e->slots)
        if (s.ticket == ticket) {
            HIP_TRY(hipSetDevice(e->device));
            HIP_TRY(hipEventSynchronize(s.copied));
            return PSSBAM_OK;
        }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_submit(pssbam_engine *e, const void *records, uint64_t nbytes, const uint32_t *offsets,
                                    uint32_t n_records) {
    uint64_t ticket = 0;
    int rc = pssbam_engine_submit_async(e, records, nbytes, offsets, n_records, &ticket);
    if (rc) return rc;
    // contract: the caller's buffers are free for reuse when we return
    return pssbam_engine_wait_copied(e, ticket);
}

extern "C" int pssbam_engine_phase_times(pssbam_engine *e, double *h2d_ms, uint64_t *h2d_bytes, double *kernel_ms,
                                         uint64_t *n_launches) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    for (Slot &s : e->slots) book_copy_time(e, s);
    rc = resolve_launch_events(e);
    if (rc) return rc;
    if (h2d_ms) *h2d_ms = e->h2d_ms;
    if (h2d_bytes) *h2d_bytes = e->h2d_bytes;
    if (kernel_ms) *kernel_ms = e->kernel_ms;
    if (n_launches) *n_launches = e->kernel_launches;
    return PSSBAM_OK;
}

static int feed_flush(pssbam_engine *e);

extern "C" int pssbam_engine_sync(pssbam_engine *e) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    {
        const int rc = feed_flush(e);   // compressed blocks still being collected (pssbam_engine_submit_bgzf)
        if (rc) return rc;
    }
    if (e->copy_stream2) HIP_TRY(hipStreamSynchronize(e->copy_stream2));
    if (e->copy_stream) HIP_TRY(hipStreamSynchronize(e->copy_stream));
    if (e->genome_stream) HIP_TRY(hipStreamSynchronize(e->genome_stream));
    for (hipStream_t q : e->inflate_stream)
        if (q) HIP_TRY(hipStreamSynchronize(q));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int rc = genome_settle(e);
    if (rc) return rc;
    if (!e->sel_queue.empty())   // the record sink: everything outstanding is delivered before sync returns
        if (const int rs = select_poll(e, true)) return rs;
    if (const int rs = select_report(e)) return rs;
    // (the streams are quiet either way: the caller's buffers are free)
    if (!e->deferred.empty())
        return fail(PSSBAM_ESTATE, "compressed blocks were fed (pssbam_engine_feed_open) but set_genome / set_references never followed");
    return PSSBAM_OK;
}

// -A: f(plane, words) for every touched plane among first .. first + n - 1, its 2 * rows * 16 words on the host.  The touched
// words are read first and the planes copied in runs of touched neighbours, so a block of 10^6 planes of which a few
// hundred hold something costs a few hundred small copies.  (The stream is quiet: the caller has synced.)
template <class F>
static int for_touched_planes(pssbam_engine *e, uint32_t first, uint32_t n, F f) {
    if (!n) return PSSBAM_OK;
    std::vector<unsigned long long> flag(n), buf;
    HIP_TRY(hipMemcpy(flag.data(), e->d_counters + e->off_touched + first, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const uint32_t max_run = std::max<uint32_t>(1u, (8u << 20) / e->plane_words);   // at most 64 MiB a copy
    for (uint32_t i = 0; i < n;) {
        if (!flag[i]) { i++; continue; }
        uint32_t j = i + 1;
        while (j < n && flag[j] && j - i < max_run) j++;
        buf.resize((size_t)(j - i) * e->plane_words);
        HIP_TRY(hipMemcpy(buf.data(), e->d_counters + e->off_groups + (uint64_t)(first + i) * e->plane_words, buf.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
        for (uint32_t k = i; k < j; k++) f(first + k, buf.data() + (size_t)(k - i) * e->plane_words);
        i = j;
    }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish(pssbam_engine *e, unsigned long *fwd, unsigned long *rev, uint64_t *k5,
                                    uint64_t *k3, uint64_t stats[PSSBAM_ST_N]) {
    int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    static_assert(sizeof(unsigned long) == 8, "LP64 expected");
    const size_t tab = (size_t)e->rows * 16;
    if (e->per_contig) {   // -A: the totals are the sum of the touched planes; the rest of the block is not read back
        std::vector<unsigned long long> h(e->off_groups), sum(2 * tab, 0ull);
        HIP_TRY(hipMemcpy(h.data(), e->d_counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        rc = for_touched_planes(e, 0, e->n_planes, [&](uint32_t, const unsigned long long *p) {
            for (size_t i = 0; i < 2 * tab; i++) sum[i] += p[i];
        });
        if (rc) return rc;
        if (fwd) for (size_t i = 0; i < tab; i++) fwd[i] = (unsigned long)(h[i] + sum[i]);
        if (rev) for (size_t i = 0; i < tab; i++) rev[i] = (unsigned long)(h[e->off_rev + i] + sum[tab + i]);
        if (stats) for (int i = 0; i < PSSBAM_ST_N; i++) stats[i] = h[e->off_stats + i];
        return PSSBAM_OK;
    }
    std::vector<unsigned long long> h(e->n_counters);
    HIP_TRY(hipMemcpy(h.data(), e->d_counters, e->n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // -G / -S: the totals are every plane's sum (plane 0, the unassigned bucket, sits where an ungrouped engine keeps its tables)
    for (size_t g = 0; g < e->n_planes; g++)
        for (size_t i = 0; i < 2 * tab; i++) h[i] += h[e->off_groups + g * e->plane_words + i];
    // k-mer planes: the same for the leading [k5 | k3]
    for (size_t g = 0; g < e->n_planes && e->kplane_words; g++)
        for (uint64_t i = 0; i < e->kplane_words; i++) h[e->off_k5 + i] += h[(uint64_t)e->off_groups + g * e->kplane_words + i];
    if (fwd) for (size_t i = 0; i < tab; i++) fwd[i] = (unsigned long)h[i];
    if (rev) for (size_t i = 0; i < tab; i++) rev[i] = (unsigned long)h[e->off_rev + i];
    if (k5) for (uint64_t i = 0; i < e->n_bins; i++) k5[i] = h[e->off_k5 + i];
    if (k3) for (uint64_t i = 0; i < e->n_bins; i++) k3[i] = h[e->off_k3 + i];
    if (stats) for (int i = 0; i < PSSBAM_ST_N; i++) stats[i] = h[e->off_stats + i];
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_groups(pssbam_engine *e, int32_t group, unsigned long *fwd, unsigned long *rev) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (e->cfg.tally_mask == PSSBAM_TALLY_KMER) return fail(PSSBAM_EINVAL, "a k-mer engine's planes are read with pssbam_engine_finish_kmer_groups");
    const int32_t n_planes = (int32_t)e->n_planes;
    if (!n_planes) return fail(PSSBAM_ESTATE, "none of pssbam_engine_set_read_groups / _set_length_bins / _set_contig_sets / _set_per_contig / _set_replicates has been called");
    if (group < -1 || group >= n_planes) return fail(PSSBAM_EINVAL, "group %d outside -1..%d", group, n_planes - 1);
    int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t tab = (size_t)e->rows * 16;
    const size_t at = group < 0 ? 0 : e->off_groups + (size_t)group * e->plane_words;
    std::vector<unsigned long long> h(2 * tab);
    HIP_TRY(hipMemcpy(h.data(), e->d_counters + at, 2 * tab * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (fwd) for (size_t i = 0; i < tab; i++) fwd[i] = (unsigned long)h[i];
    if (rev) for (size_t i = 0; i < tab; i++) rev[i] = (unsigned long)h[tab + i];
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_kmer_groups(pssbam_engine *e, int32_t group, uint64_t *k5, uint64_t *k3) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (e->cfg.tally_mask != PSSBAM_TALLY_KMER) return fail(PSSBAM_EINVAL, "only a k-mer engine (PSSBAM_TALLY_KMER alone) has k-mer planes");
    const int32_t n_planes = (int32_t)e->n_planes;
    if (!n_planes) return fail(PSSBAM_ESTATE, "none of pssbam_engine_set_read_groups / _set_length_bins / _set_contig_sets has been called");
    if (group < -1 || group >= n_planes) return fail(PSSBAM_EINVAL, "group %d outside -1..%d", group, n_planes - 1);
    int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const uint64_t at = group < 0 ? (uint64_t)e->off_k5 : (uint64_t)e->off_groups + (uint64_t)group * e->kplane_words;
    if (k5) HIP_TRY(hipMemcpy(k5, e->d_counters + at, e->n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (k3) HIP_TRY(hipMemcpy(k3, e->d_counters + at + e->n_bins, e->n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSSBAM_OK;
}

// What every setter that switches `mine` on asks first: no other mode is on (setting the one that is on again is no conflict)
static int check_exclusive(const pssbam_engine *e, Mode mine) {
    for (size_t m = 0; m < sizeof MODES / sizeof *MODES; m++)
        if (m != (size_t)mine && MODES[m].on(e)) return fail(PSSBAM_EINVAL, "%s and %s exclude each other", MODES[mine].name, MODES[m].name);
    return PSSBAM_OK;
}

// What the setters that resize the counter block require: nothing tallied yet, and the block is the engine's own.  `what`
// names what is being set in the messages.
static int check_may_resize(const pssbam_engine *e, const char *what) {
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set %s after create or reset, before the first tally", what);
    if (e->d_counters != e->d_counters_own) return fail(PSSBAM_ESTATE, "a caller-bound counter block cannot grow: set %s before bind_counters", what);
    return PSSBAM_OK;
}

// The counter block becomes n_counters words (more or fewer than before), zeroed: nothing has been counted yet.  The old
// block may still be named by work queued on the stream (the compressed feed): it is retired, not freed.
static int grow_counters(pssbam_engine *e, uint64_t n_counters) {
    unsigned long long *d_counters = nullptr;
    HIP_TRY(hipMalloc(&d_counters, n_counters * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_counters, 0, n_counters * sizeof(unsigned long long), e->stream));
    if (e->d_counters_own) e->retired.push_back(e->d_counters_own);
    e->d_counters = e->d_counters_own = d_counters;
    e->n_counters = n_counters;
    return PSSBAM_OK;
}

// The exclusive modes' extra words: the block becomes off_groups + words long (it grows, or shrinks back), zeroed.
static int resize_extra(pssbam_engine *e, uint64_t words, const char *what) {
    if (const int rc = check_may_resize(e, what)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t n_counters = (uint64_t)e->off_groups + words;
    if (n_counters > 0xFFFFFFFFull) return fail(PSSBAM_EINVAL, "the counter block would pass 2^32 words");
    return grow_counters(e, n_counters);
}

// What set_read_groups, set_length_bins, set_contig_sets and set_replicates share: the counter block grows to n_planes [fwd | rev] planes
// (a k-mer engine: [k5 | k3]) behind the stats.  `what` names the caller's planes in the messages.
static int set_planes(pssbam_engine *e, PlaneSel sel, Mode mode, uint32_t n_planes) {
    const char *what = MODES[mode].name;
    if (const int rc = check_exclusive(e, mode)) return rc;
    const bool kmer = e->cfg.tally_mask == PSSBAM_TALLY_KMER;
    if (e->cfg.tally_mask != PSSBAM_TALLY_PSS && !kmer)
        return fail(PSSBAM_EINVAL, "%s split the substitution tables or the k-mer tables, not both (PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER)", what);
    if (const int rc = check_may_resize(e, what)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    // 64-bit throughout: a k-mer plane is 2 * 4^k words (2^31 at k = 15)
    const uint64_t n_counters = (uint64_t)e->off_groups + (uint64_t)n_planes * (kmer ? e->kplane_words : (uint64_t)e->plane_words);
    if (kmer) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (n_counters * sizeof(unsigned long long) > (uint64_t)free_b)
            return fail(PSSBAM_ENOMEM, "k = %d with %u planes (plane 0 and %u %s) needs a counter block of %llu bytes; the device has %llu free",
                        e->cfg.kmer.klen, n_planes + 1u, n_planes, what, (unsigned long long)(n_counters * sizeof(unsigned long long)),
                        (unsigned long long)free_b);
    }
    if (const int rc = grow_counters(e, n_counters)) return rc;
    e->planes = sel;
    e->n_planes = n_planes;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_read_groups(pssbam_engine *e, int32_t n, const char *const *ids) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (n < 1 || n > PSSBAM_MAX_READ_GROUPS || !ids) return fail(PSSBAM_EINVAL, "read group count %d outside 1..%d", n, PSSBAM_MAX_READ_GROUPS);
    if (e->has_rg) return fail(PSSBAM_EINVAL, "read groups and a -R read group filter exclude each other");
    for (int32_t i = 0; i < n; i++)
        if (!ids[i]) return fail(PSSBAM_EINVAL, "read group %d is NULL", i);
    // ID table (concatenated) + open-addressing hash over it; a repeated ID keeps its first index
    std::vector<std::string> groups(ids, ids + n);
    std::string cat;
    std::vector<uint32_t> offs(1, 0u);
    for (const std::string &g : groups) {
        cat += g;
        offs.push_back((uint32_t)cat.size());
    }
    uint32_t hsize = 16;
    while (hsize < 2u * (uint32_t)n) hsize <<= 1;
    std::vector<uint32_t> hash(hsize, 0u);
    for (int32_t g = 0; g < n; g++) {
        uint32_t hv = FNV1A_SEED;
        for (unsigned char ch : groups[g]) hv = fnv1a_step(hv, ch);
        for (uint32_t k = 0;; k++) {
            uint32_t &slot = hash[(hv + k) & (hsize - 1)];
            if (slot == 0u) { slot = (uint32_t)g + 1u; break; }
            if (groups[slot - 1u] == groups[g]) break;   // duplicate: the first one counts
        }
    }
    // on the device before the counter block grows: the engine never sees planes without their ID table.  The old tables
    // are retired, not freed, like the old counter block.
    HIP_TRY(hipSetDevice(e->device));
    uint8_t *d_ids = nullptr;
    uint32_t *d_offs = nullptr, *d_hash = nullptr;
    HIP_TRY(hipMalloc(&d_ids, cat.size() + 16));
    HIP_TRY(hipMalloc(&d_offs, offs.size() * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_hash, hash.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(d_ids, cat.data(), cat.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_offs, offs.data(), offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_hash, hash.data(), hash.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (const int rc = set_planes(e, PLANES_RG, MODE_RG, (uint32_t)n)) {
        for (void *p : {(void *)d_ids, (void *)d_offs, (void *)d_hash}) (void)hipFree(p);
        return rc;
    }
    for (void *old : {(void *)e->d_grp_ids, (void *)e->d_grp_offs, (void *)e->d_grp_hash})
        if (old) e->retired.push_back(old);
    e->d_grp_ids = d_ids;
    e->d_grp_offs = d_offs;
    e->d_grp_hash = d_hash;
    e->grp_hash_mask = hsize - 1;
    e->dev_pieces = 0;   // whole records are staged from now on: resampled at the next launch
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_min_base_quality(pssbam_engine *e, int32_t q) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (q < 0 || q > PSSBAM_MAX_BASE_QUALITY) return fail(PSSBAM_EINVAL, "minimum base quality %d outside 0..%d", q, PSSBAM_MAX_BASE_QUALITY);
    if (!(e->cfg.tally_mask & PSSBAM_TALLY_PSS)) return fail(PSSBAM_EINVAL, "base qualities mask the substitution tables: the engine needs PSSBAM_TALLY_PSS");
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set the minimum base quality after create or reset, before the first tally");
    if ((e->min_bq > 0) != (q > 0)) e->dev_pieces = 0;   // whole records or prefixes are staged from now on: resampled at the next launch
    e->min_bq = (uint32_t)q;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_gapped_reads(pssbam_engine *e, int32_t on) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (on) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "gapped reads are tallied by their anchored ends in the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        if (const int rc = check_exclusive(e, MODE_GAPPED)) return rc;
        if (e->dedup) return fail(PSSBAM_EINVAL, "gapped reads do not go with duplicate flagging (pssbam_engine_set_duplicates): the key of a clipped read is not defined");
        if (e->coverage) return fail(PSSBAM_EINVAL, "gapped reads do not go with coverage (pssbam_engine_set_coverage): the span of a clipped or gapped read is not defined");
        if (e->has_sites) return fail(PSSBAM_EINVAL, "gapped reads do not go with sites (pssbam_engine_set_sites): the offsets of a clipped or gapped read need a CIGAR walk");
    }
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set gapped reads after create or reset, before the first tally");
    e->gapped = on != 0;   // (the counter block keeps its size: a caller-bound block stays bound)
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_length_histogram(pssbam_engine *e, int32_t max_len) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (max_len < 0 || max_len > PSSBAM_MAX_HIST_LENGTH) return fail(PSSBAM_EINVAL, "length histogram limit %d outside 0..%d", max_len, PSSBAM_MAX_HIST_LENGTH);
    if (!(e->cfg.tally_mask & PSSBAM_TALLY_PSS))
        return fail(PSSBAM_EINVAL, "the length histogram counts the reads added to the substitution tables: the engine needs PSSBAM_TALLY_PSS");
    if (max_len)
        if (const int rc = check_exclusive(e, MODE_HIST)) return rc;
    if ((uint32_t)max_len == e->hist_max) return check_may_resize(e, "the length histogram");
    if (const int rc = resize_extra(e, max_len ? 2ull * ((uint64_t)max_len + 2ull) : 0ull, "the length histogram")) return rc;
    e->hist_max = (uint32_t)max_len;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_length_histogram(pssbam_engine *e, uint64_t *fwd, uint64_t *rev) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->hist_max) return fail(PSSBAM_EINVAL, "pssbam_engine_set_length_histogram has not been called");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t n = (size_t)e->hist_max + 2;
    if (fwd) HIP_TRY(hipMemcpy(fwd, e->d_counters + e->off_groups, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rev) HIP_TRY(hipMemcpy(rev, e->d_counters + e->off_groups + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_mismatches(pssbam_engine *e, int32_t hist_max, int32_t max_mismatches, int32_t transversions_only) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (hist_max < 0 || hist_max > PSSBAM_MAX_MISMATCHES) return fail(PSSBAM_EINVAL, "mismatch histogram limit %d outside 0..%d", hist_max, PSSBAM_MAX_MISMATCHES);
    if (max_mismatches < -1 || max_mismatches > PSSBAM_MAX_MISMATCHES)
        return fail(PSSBAM_EINVAL, "maximum mismatch count %d outside -1..%d", max_mismatches, PSSBAM_MAX_MISMATCHES);
    const bool on = hist_max > 0 || max_mismatches >= 0;
    if (on) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "the mismatch count filters the reads of the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        if (e->cfg.pss.region_len > 30)
            return fail(PSSBAM_EINVAL, "the mismatch count needs a region length of at most 30 (the decision is taken in the one pass that holds all rows), not %d", e->cfg.pss.region_len);
        if (const int rc = check_exclusive(e, MODE_MISM)) return rc;
    }
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set the mismatch count after create or reset, before the first tally");
    if ((uint32_t)hist_max != e->mism_hist)
        if (const int rc = resize_extra(e, hist_max ? 2ull * ((uint64_t)hist_max + 2ull) : 0ull, "the mismatch histogram")) return rc;
    e->mism_hist = (uint32_t)hist_max;
    e->mism_max = max_mismatches;
    e->mism_tv = on && transversions_only != 0;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_mismatches(pssbam_engine *e, uint64_t *fwd, uint64_t *rev) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->mism_hist) return fail(PSSBAM_EINVAL, "pssbam_engine_set_mismatches has not been called with a histogram limit");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t n = (size_t)e->mism_hist + 2;
    if (fwd) HIP_TRY(hipMemcpy(fwd, e->d_counters + e->off_groups, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rev) HIP_TRY(hipMemcpy(rev, e->d_counters + e->off_groups + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_interior(pssbam_engine *e, int32_t margin) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (margin < -1 || margin > PSSBAM_MAX_INTERIOR_MARGIN) return fail(PSSBAM_EINVAL, "interior margin %d outside -1..%d", margin, PSSBAM_MAX_INTERIOR_MARGIN);
    if (margin >= 0) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "the interior table counts the reads of the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        if (e->cfg.pss.region_len > 30)
            return fail(PSSBAM_EINVAL, "the interior table needs a region length of at most 30 (a read's fate is decided in the one pass that holds all rows), not %d", e->cfg.pss.region_len);
        if (const int rc = check_exclusive(e, MODE_INTERIOR)) return rc;
    }
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set the interior table after create or reset, before the first tally");
    if ((margin >= 0) != interior_on(e))
        if (const int rc = resize_extra(e, margin >= 0 ? (uint64_t)INTERIOR_WORDS : 0ull, "the interior table")) return rc;
    e->interior_margin = margin;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_interior(pssbam_engine *e, uint64_t table[16], uint64_t *reads) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!interior_on(e)) return fail(PSSBAM_EINVAL, "pssbam_engine_set_interior has not been called with a margin");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    if (table) HIP_TRY(hipMemcpy(table, e->d_counters + e->off_groups, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reads) HIP_TRY(hipMemcpy(reads, e->d_counters + e->off_groups + 16, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_composition(pssbam_engine *e, int32_t width) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (width < 0 || width > PSSBAM_MAX_COMPOSITION) return fail(PSSBAM_EINVAL, "composition width %d outside 0..%d", width, PSSBAM_MAX_COMPOSITION);
    if (width > 0) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "the composition table counts the reads of the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        if (e->cfg.pss.region_len > 30)
            return fail(PSSBAM_EINVAL, "the composition table needs a region length of at most 30 (a read's fate and its end windows are those of the one pass that holds all rows), not %d", e->cfg.pss.region_len);
        if (const int rc = check_exclusive(e, MODE_COMPOSITION)) return rc;
    }
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set the composition table after create or reset, before the first tally");
    if ((uint32_t)width != e->composition)
        if (const int rc = resize_extra(e, 20ull * (uint64_t)width, "the composition table")) return rc;
    e->composition = (uint32_t)width;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_composition(pssbam_engine *e, uint64_t *c5, uint64_t *c3) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!composition_on(e)) return fail(PSSBAM_EINVAL, "pssbam_engine_set_composition has not been called with a width");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t words = 10u * (size_t)e->composition;
    if (c5) HIP_TRY(hipMemcpy(c5, e->d_counters + e->off_groups, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (c3) HIP_TRY(hipMemcpy(c3, e->d_counters + e->off_groups + words, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_read_score(pssbam_engine *e, const int16_t *weights, int32_t n_dist, int32_t n_qual, int32_t use_filter,
                                            int32_t min_score, int32_t hist_half, int32_t hist_shift) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    const bool on = weights != nullptr;
    if (!on) n_dist = n_qual = use_filter = min_score = hist_half = hist_shift = 0;
    if (on) {
        if (n_dist < 1 || n_dist > PSSBAM_MAX_SCORE_DIST) return fail(PSSBAM_EINVAL, "read score: %d distances outside 1..%d", n_dist, PSSBAM_MAX_SCORE_DIST);
        if (n_qual < 1 || n_qual > PSSBAM_MAX_SCORE_QUAL) return fail(PSSBAM_EINVAL, "read score: %d quality columns outside 1..%d", n_qual, PSSBAM_MAX_SCORE_QUAL);
        if (hist_half < 0 || hist_half > PSSBAM_MAX_SCORE_HALF) return fail(PSSBAM_EINVAL, "read score: histogram half width %d outside 0..%d", hist_half, PSSBAM_MAX_SCORE_HALF);
        if (hist_shift < 0 || hist_shift > 16) return fail(PSSBAM_EINVAL, "read score: histogram shift %d outside 0..16", hist_shift);
        for (int32_t i = 0; i < 4 * n_dist * n_qual; i++)
            if (weights[i] < -PSSBAM_MAX_SCORE_WEIGHT || weights[i] > PSSBAM_MAX_SCORE_WEIGHT)
                return fail(PSSBAM_EINVAL, "read score: weight %d (entry %d) beyond +-%d", (int)weights[i], i, PSSBAM_MAX_SCORE_WEIGHT);
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "the read score filters the reads of the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        if (e->cfg.pss.region_len > 30)
            return fail(PSSBAM_EINVAL, "the read score needs a region length of at most 30 (the decision is taken in the one pass that holds all rows), not %d", e->cfg.pss.region_len);
        if (const int rc = check_exclusive(e, MODE_SCORE)) return rc;
    }
    if (e->tallied) return fail(PSSBAM_ESTATE, "records have been tallied already: set the read score after create or reset, before the first tally");
    HIP_TRY(hipSetDevice(e->device));
    int16_t *d_w = nullptr;
    if (on) {   // the weights go to the device here; an earlier table may still be named by nothing (nothing has been tallied)
        const size_t bytes = (size_t)4 * (size_t)n_dist * (size_t)n_qual * sizeof(int16_t);
        HIP_TRY(hipMalloc(&d_w, bytes));
        if (hipMemcpy(d_w, weights, bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d_w);
            return fail(PSSBAM_EHIP, "read score: the weights could not be copied to the device");
        }
    }
    if ((uint32_t)hist_half != e->score_half)
        if (const int rc = resize_extra(e, 4ull * (uint64_t)hist_half, "the read-score histogram")) {
            if (d_w) (void)hipFree(d_w);
            return rc;
        }
    if (e->d_score_w) (void)hipFree(e->d_score_w);
    e->d_score_w = d_w;
    e->score_nd = (uint32_t)n_dist;
    e->score_nq = (uint32_t)n_qual;
    e->score_filter = use_filter != 0;
    e->score_min = min_score;
    e->score_half = (uint32_t)hist_half;
    e->score_shift = (uint32_t)hist_shift;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_read_score(pssbam_engine *e, uint64_t *fwd, uint64_t *rev) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->score_half) return fail(PSSBAM_EINVAL, "pssbam_engine_set_read_score has not been called with a histogram");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t n = 2u * (size_t)e->score_half;
    if (fwd) HIP_TRY(hipMemcpy(fwd, e->d_counters + e->off_groups, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rev) HIP_TRY(hipMemcpy(rev, e->d_counters + e->off_groups + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_site_context(pssbam_engine *e, int32_t mode) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (mode != PSSBAM_SITE_NONE && mode != PSSBAM_SITE_CPG) return fail(PSSBAM_EINVAL, "unknown site context %d", mode);
    if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
        return fail(PSSBAM_EINVAL, "site context splits the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
    if (mode != PSSBAM_SITE_NONE)
        if (const int rc = check_exclusive(e, MODE_SITE)) return rc;
    if ((uint32_t)mode == e->site_mode) return check_may_resize(e, "the site context");
    if (const int rc = resize_extra(e, mode ? 2ull * e->rows * 16ull : 0ull, "the site context")) return rc;
    e->site_mode = (uint32_t)mode;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_site_context(pssbam_engine *e, unsigned long *fwd_in, unsigned long *rev_in) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->site_mode) return fail(PSSBAM_EINVAL, "pssbam_engine_set_site_context has not been called");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    std::vector<unsigned long long> h(e->n_counters);
    HIP_TRY(hipMemcpy(h.data(), e->d_counters, e->n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const size_t tab = (size_t)e->rows * 16;
    // rows 0 and 1 (the context bases) are never masked: they stay zero on the device and are T's here
    for (size_t i = 0; i < tab; i++) {
        if (fwd_in) fwd_in[i] = (unsigned long)(i < 32 ? h[i] : h[e->off_groups + i]);
        if (rev_in) rev_in[i] = (unsigned long)(i < 32 ? h[e->off_rev + i] : h[e->off_groups + tab + i]);
    }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_end_condition(pssbam_engine *e, int32_t depth, int32_t cell5, int32_t cell3) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (depth < 0 || depth > PSSBAM_MAX_END_DEPTH) return fail(PSSBAM_EINVAL, "end condition depth %d outside 0..%d", depth, PSSBAM_MAX_END_DEPTH);
    if (depth && (cell5 < 0 || cell5 > 15 || cell3 < 0 || cell3 > 15)) return fail(PSSBAM_EINVAL, "end condition cells %d, %d outside 0..15", cell5, cell3);
    if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
        return fail(PSSBAM_EINVAL, "the end condition splits the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
    if (depth > e->cfg.pss.region_len) return fail(PSSBAM_EINVAL, "end condition depth %d beyond the region length %d", depth, e->cfg.pss.region_len);
    if (depth && e->cfg.pss.region_len > 30)
        return fail(PSSBAM_EINVAL, "the end condition needs a region length of at most 30 (one 32-row pass holds both ends' marks), not %d", e->cfg.pss.region_len);
    if (depth)
        if (const int rc = check_exclusive(e, MODE_END)) return rc;
    // (the pair and its read counters)
    if (const int rc = (uint32_t)depth != e->end_depth ? resize_extra(e, depth ? 2ull * e->rows * 16ull + 4ull : 0ull, "the end condition")
                                                       : check_may_resize(e, "the end condition")) return rc;
    e->end_depth = (uint32_t)depth;
    e->end_cell5 = depth ? (uint32_t)cell5 : 0u;
    e->end_cell3 = depth ? (uint32_t)cell3 : 0u;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_end_condition(pssbam_engine *e, unsigned long *fwd_c, unsigned long *rev_c, uint64_t reads[4]) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->end_depth) return fail(PSSBAM_EINVAL, "pssbam_engine_set_end_condition has not been called");
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t tab = (size_t)e->rows * 16;
    std::vector<unsigned long long> h(2 * tab + 4);
    HIP_TRY(hipMemcpy(h.data(), e->d_counters + e->off_groups, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tab; i++) {
        if (fwd_c) fwd_c[i] = (unsigned long)h[i];
        if (rev_c) rev_c[i] = (unsigned long)h[tab + i];
    }
    if (reads) for (int k = 0; k < 4; k++) reads[k] = h[2 * tab + k];
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_length_bins(pssbam_engine *e, int32_t n_edges, const uint32_t *edges) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (n_edges < 1 || n_edges > PSSBAM_MAX_LENGTH_BINS - 1 || !edges)
        return fail(PSSBAM_EINVAL, "length bin edge count %d outside 1..%d", n_edges, PSSBAM_MAX_LENGTH_BINS - 1);
    // l < e1 < ... < ek <= L: every bin [l, e1-1], [e1, e2-1], ..., [ek, L] is a non-empty -l / -L window
    // (a k-mer engine: the window of fragkon's -l / -L, compared with strlen(SEQ))
    const bool kmer = e->cfg.tally_mask == PSSBAM_TALLY_KMER;
    const uint64_t lo = kmer ? e->cfg.kmer.min_read_len : e->cfg.pss.min_read_len, hi = kmer ? e->cfg.kmer.max_read_len : e->cfg.pss.max_read_len;
    for (int32_t i = 0; i < n_edges; i++) {
        const uint64_t prev = i ? (uint64_t)edges[i - 1] : lo;
        if (edges[i] <= prev || edges[i] > hi)
            return fail(PSSBAM_EINVAL, "length bin edge %d (%u) must lie above %llu and at most at %llu", i, edges[i],
                        (unsigned long long)prev, (unsigned long long)hi);
    }
    const int rc = set_planes(e, PLANES_LEN, MODE_LEN, (uint32_t)n_edges + 1u);
    if (rc) return rc;
    e->len_edges.assign(edges, edges + n_edges);
    return PSSBAM_OK;
}

// -J: K read-name replicates, planes 1 .. K of the -S layout (plane 0 stays empty); k = 0: the block and the launches of an
// engine that never had the setting
extern "C" int pssbam_engine_set_replicates(pssbam_engine *e, int32_t k) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (k < 0 || k == 1 || k > PSSBAM_MAX_REPLICATES) return fail(PSSBAM_EINVAL, "replicate count %d outside 2..%d (0 = off)", k, PSSBAM_MAX_REPLICATES);
    if (k) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "replicates split the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        return set_planes(e, PLANES_HASH, MODE_HASH, (uint32_t)k);   // (the other modes: refused there)
    }
    if (e->planes != PLANES_HASH) return check_may_resize(e, "replicates");
    if (const int rc = resize_extra(e, 0, "replicates")) return rc;
    e->planes = PLANES_NONE;
    e->n_planes = 0;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_contig_sets(pssbam_engine *e, int32_t n_sets, int64_t n_names, const char *const *names,
                                             const int32_t *set_of) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (n_sets < 1 || n_sets > PSSBAM_MAX_CONTIG_SETS)
        return fail(PSSBAM_EINVAL, "contig set count %d outside 1..%d", n_sets, PSSBAM_MAX_CONTIG_SETS);
    if (n_names < 0 || (n_names && (!names || !set_of))) return fail(PSSBAM_EINVAL, "bad contig name list");
    std::unordered_map<std::string, uint32_t> plane;
    plane.reserve((size_t)n_names);
    for (int64_t i = 0; i < n_names; i++) {
        if (!names[i]) return fail(PSSBAM_EINVAL, "contig name %lld is NULL", (long long)i);
        if (set_of[i] < 0 || set_of[i] >= n_sets)
            return fail(PSSBAM_EINVAL, "contig %s: set %d outside 0..%d", names[i], set_of[i], n_sets - 1);
        const auto ins = plane.emplace(names[i], (uint32_t)set_of[i] + 1u);
        if (!ins.second && ins.first->second != (uint32_t)set_of[i] + 1u)
            return fail(PSSBAM_EINVAL, "contig %s is given under two sets (%u and %d)", names[i], ins.first->second - 1u, set_of[i]);
    }
    const int rc = set_planes(e, PLANES_REF, MODE_REF, (uint32_t)n_sets);
    if (rc) return rc;
    e->ctg_plane.swap(plane);
    if (!e->have_refs) return PSSBAM_OK;   // set_references packs the planes into ref_info when it comes
    // the reference table is there already: built again with the planes (nothing has read it: no tally yet)
    const std::vector<std::string> refs = e->ref_names;
    std::vector<const char *> ptrs(refs.size());
    for (size_t i = 0; i < refs.size(); i++) ptrs[i] = refs[i].c_str();
    return pssbam_engine_set_references(e, e->n_ref, ptrs.data());
}

// -A: the counter block for n_ref references: [fwd | rev | stats | n_ref + 1 planes | n_ref + 1 touched words].  Before the first
// tally the block is simply made anew.  Afterwards (SAM text: set_references comes again as new RNAMEs show up) the block
// grows in place of the old one: planes 0 .. old n_ref - 1 keep their offsets, the "*" plane and the touched words move.
static int size_per_contig(pssbam_engine *e, int32_t n_ref) {
    const uint32_t n_planes = (uint32_t)n_ref + 1u, old_planes = e->n_planes;
    if (n_planes == old_planes) return PSSBAM_OK;
    if (e->d_counters != e->d_counters_own)
        return fail(PSSBAM_ESTATE, "a caller-bound counter block cannot grow: per-contig tables for %d references need another size than it has", n_ref);
    if (e->tallied && n_planes < old_planes) return fail(PSSBAM_ESTATE, "records have been tallied already: the reference list can only grow");
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t plane_span = (uint64_t)n_planes * e->plane_words;   // (n_ref + 1) * 2 * (region_len + 2) * 16
    const uint64_t n_counters = (uint64_t)e->off_groups + plane_span + n_planes;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (n_counters * sizeof(unsigned long long) > (uint64_t)free_b)
        return fail(PSSBAM_ENOMEM, "per-contig tables for %d references need a counter block of %llu bytes; the device has %llu free", n_ref,
                    (unsigned long long)(n_counters * sizeof(unsigned long long)), (unsigned long long)free_b);
    const uint64_t off_touched = (uint64_t)e->off_groups + plane_span;
    if (!(e->tallied && old_planes > 0)) {   // nothing counted yet
        if (const int rc = grow_counters(e, n_counters)) return rc;
        e->n_planes = n_planes;
        e->off_touched = off_touched;
        return PSSBAM_OK;
    }
    // the counts move over; the old block is freed here, not retired: the list may grow many times, and once the stream has
    // run dry nothing names the old block any more (tally launches are never put off once references have been set)
    const size_t w = sizeof(unsigned long long);
    unsigned long long *old = e->d_counters_own, *d_new = nullptr;
    const uint64_t star_old = (uint64_t)e->off_groups + (uint64_t)(old_planes - 1u) * e->plane_words;
    HIP_TRY(hipMalloc(&d_new, n_counters * w));
    hipError_t err = hipMemsetAsync(d_new, 0, n_counters * w, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(d_new, old, star_old * w, hipMemcpyDeviceToDevice, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(d_new + off_touched - e->plane_words, old + star_old, e->plane_words * w, hipMemcpyDeviceToDevice, e->stream);
    if (err == hipSuccess && old_planes > 1u)
        err = hipMemcpyAsync(d_new + off_touched, old + e->off_touched, (old_planes - 1u) * w, hipMemcpyDeviceToDevice, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(d_new + off_touched + n_planes - 1u, old + e->off_touched + old_planes - 1u, w, hipMemcpyDeviceToDevice, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
        (void)hipFree(d_new);
        return fail(PSSBAM_EHIP, "growing the per-contig tables: %s", hipGetErrorString(err));
    }
    HIP_TRY(hipFree(old));
    e->d_counters = e->d_counters_own = d_new;
    e->n_counters = n_counters;
    e->n_planes = n_planes;
    e->off_touched = off_touched;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_set_per_contig(pssbam_engine *e, int32_t on) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (on) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS)
            return fail(PSSBAM_EINVAL, "per-contig tables split the substitution tables: the engine needs PSSBAM_TALLY_PSS alone");
        if (const int rc = check_exclusive(e, MODE_EACH)) return rc;
    }
    if (const int rc = check_may_resize(e, "per-contig tables")) return rc;
    if ((on != 0) == e->per_contig) return PSSBAM_OK;
    if (!on) {   // switched off: the block and the launches of an engine that never had the setting
        if (const int rc = resize_extra(e, 0, "per-contig tables")) return rc;
        e->per_contig = false;
        e->planes = PLANES_NONE;
        e->n_planes = 0;
        e->off_touched = 0;
        return PSSBAM_OK;
    }
    // the block is sized when the reference count is known: now, or at feed_open / set_references
    e->per_contig = true;
    e->planes = PLANES_EACH;
    e->n_planes = 0;
    const int rc = e->have_refs ? size_per_contig(e, e->n_ref) : e->feed_opened ? size_per_contig(e, e->feed_n_ref) : PSSBAM_OK;
    if (rc) {
        e->per_contig = false;
        e->planes = PLANES_NONE;
    }
    return rc;
}

extern "C" int pssbam_engine_finish_contigs(pssbam_engine *e, int32_t first_ref, int32_t n, unsigned long *fwd, unsigned long *rev, uint8_t *touched) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->per_contig) return fail(PSSBAM_ESTATE, "pssbam_engine_set_per_contig has not been called");
    if (first_ref < 0 || n < 0 || (uint64_t)first_ref + (uint64_t)n > e->n_planes)
        return fail(PSSBAM_EINVAL, "planes %d .. %lld outside 0..%d", first_ref, (long long)first_ref + n - 1, (int)e->n_planes - 1);
    const int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    const size_t tab = (size_t)e->rows * 16;
    if (fwd) memset(fwd, 0, (size_t)n * tab * sizeof(unsigned long));
    if (rev) memset(rev, 0, (size_t)n * tab * sizeof(unsigned long));
    if (touched) memset(touched, 0, (size_t)n);
    return for_touched_planes(e, (uint32_t)first_ref, (uint32_t)n, [&](uint32_t plane, const unsigned long long *p) {
        const size_t i = plane - (uint32_t)first_ref;
        if (touched) touched[i] = 1;
        if (fwd) for (size_t k = 0; k < tab; k++) fwd[i * tab + k] = (unsigned long)p[k];
        if (rev) for (size_t k = 0; k < tab; k++) rev[i * tab + k] = (unsigned long)p[tab + k];
    });
}

extern "C" int pssbam_engine_reset(pssbam_engine *e) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    if (!e->sel_queue.empty())   // the record sink: what the run so far kept still goes out
        if (const int rs = select_poll(e, true)) return rs;
    if (const int rs = select_report(e)) return rs;
    e->tallied = false;
    e->feed_fresh = true;   // a compressed stream fed from here on starts a new record chain
    e->feed_skip = 0;
    if (!e->deferred.empty()) {   // inflated ahead of the genome and now given up: the slots go back once their kernels have run
        e->deferred.clear();
        for (FeedAcc *sp : e->feed)
            if (sp->held) {
                sp->held = false;
                if (!sp->consumed) HIP_TRY(hipEventCreateWithFlags(&sp->consumed, hipEventDisableTiming));
                HIP_TRY(hipEventRecord(sp->consumed, e->stream));
            }
    }
    if (e->d_feed_tail) HIP_TRY(hipMemsetAsync(e->d_feed_tail, 0, sizeof(uint64_t), e->stream));
    if (e->d_feed_flags) HIP_TRY(hipMemsetAsync(e->d_feed_flags, 0, sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(e->d_counters, 0, e->n_counters * sizeof(unsigned long long), e->stream));
    if (e->d_dedup_state) {   // duplicate flagging: the table is empty again, at the size it has; the setting stays
        const int rd = dedup_poll(e, true);   // (a table that ran full is reported here at the latest)
        HIP_TRY(hipMemsetAsync(e->d_dedup_state, 0, sizeof(unsigned long long), e->stream));
        if (e->d_dedup) {
            hipLaunchKernelGGL(dedup_clear, dim3(dedup_grid(e, e->dedup_cap)), dim3(256), 0, e->stream, e->d_dedup, e->dedup_cap);
            HIP_TRY(hipGetLastError());
            e->dedup_launches++;
        }
        e->dedup_known = e->dedup_known_at = e->dedup_reading_at = e->dedup_submitted = 0;
        e->dedup_seq = 0;
        if (rd) return rd;
    }
    if (e->d_cov) {   // coverage: all zero again, at the size it has; the setting stays
        HIP_TRY(hipMemsetAsync(e->d_cov, 0, e->cov_len * sizeof(uint32_t), e->stream));
        e->cov_totals_valid = false;
    }
    if (e->d_site_counts)   // allele counts: all zero again; the sites stay
        HIP_TRY(hipMemsetAsync(e->d_site_counts, 0, e->site_idx.size() * ALLELE_WORDS * sizeof(uint32_t), e->stream));
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// allele counts at listed sites (allele_kernels.h): the finish
// --------------------------------------------------------------------------------------
extern "C" int pssbam_engine_finish_sites(pssbam_engine *e, uint64_t cap, int32_t *ref, uint32_t *pos0, uint8_t *ref_base, uint32_t *counts,
                                          uint64_t *n_sites, uint64_t totals[4]) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->has_sites) return fail(PSSBAM_EINVAL, "no sites are set (pssbam_engine_set_sites)");
    if (const int rc = pssbam_engine_sync(e)) return rc;
    const size_t n = e->d_site_idx ? e->site_idx.size() : 0;
    if (n_sites) *n_sites = n;
    const bool arrays = ref || pos0 || ref_base || counts;
    if (arrays && cap < n) return fail(PSSBAM_EINVAL, "room for %llu sites, %llu are resolved", (unsigned long long)cap, (unsigned long long)n);
    if (totals) {
        totals[0] = e->sites_given;
        totals[1] = n;
        totals[2] = totals[3] = 0;
    }
    if (!n || (!arrays && !totals)) return PSSBAM_OK;
    for (size_t j = 0; j < n; j++) {
        if (ref) ref[j] = e->site_ref[j];
        if (pos0) pos0[j] = e->site_pos[j];
    }
    if (ref_base) {
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)e->n_cu * 8));
        hipLaunchKernelGGL(allele_ref_base, dim3(grid), dim3(256), 0, e->stream, (const uint8_t *)e->d_genome, e->genome_bytes, (const uint64_t *)e->d_site_idx,
                           (uint32_t)n, e->d_site_base);
        HIP_TRY(hipGetLastError());
        std::vector<uint8_t> h(n);
        HIP_TRY(hipMemcpyAsync(h.data(), e->d_site_base, n, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t j = 0; j < n; j++) ref_base[j] = h[e->site_slot[j]];
    }
    if (counts || totals) {   // the device's rows are in the genome's order, the caller's by refID then position
        std::vector<uint32_t> h(n * ALLELE_WORDS);
        HIP_TRY(hipMemcpyAsync(h.data(), e->d_site_counts, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t j = 0; j < n; j++) {
            const uint32_t *row = &h[(size_t)e->site_slot[j] * ALLELE_WORDS];
            uint64_t sum = 0;
            for (uint32_t w = 0; w < ALLELE_WORDS; w++) sum += row[w];
            if (counts) memcpy(counts + j * ALLELE_WORDS, row, ALLELE_WORDS * sizeof(uint32_t));
            if (totals) {
                totals[2] += sum != 0;
                totals[3] += sum;
            }
        }
    }
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// depth of coverage of the kept records (coverage_kernels.h)
// --------------------------------------------------------------------------------------
// what the array is expected to take, from the caller's hint: 4 bytes per position, and per contig the padding and the rounding of
// genome_upload's layout (bgzf_api.h takes it out of the feed's memory budget)
static uint64_t coverage_reserve_bytes(const pssbam_engine *e) {
    if (!e->coverage) return 0;
    const uint64_t n_ref = e->feed_opened ? (uint64_t)std::max(e->feed_n_ref, 0) : 0ull;
    return sizeof(uint32_t) * (e->cov_hint + (n_ref + 1) * (CONTIG_PAD + CONTIG_ALIGN) + COV_TILE);
}

// the array for a genome of genome_bytes stored positions; the caller zeroes it
static int coverage_array(pssbam_engine *e, uint64_t genome_bytes) {
    e->cov_totals_valid = false;
    const uint64_t len = (genome_bytes + COV_TILE - 1) / COV_TILE * COV_TILE;
    if (e->d_cov && e->cov_len != len) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipFree(e->d_cov));
        e->d_cov = nullptr;
        e->cov_len = 0;
    }
    if (!e->d_cov) {
        if (hipMalloc((void **)&e->d_cov, len * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            e->d_cov = nullptr;
            return fail(PSSBAM_ENOMEM, "the coverage array of %llu positions (%llu bytes) does not fit the device", (unsigned long long)len,
                        (unsigned long long)(len * sizeof(uint32_t)));
        }
        e->cov_len = len;
    }
    return PSSBAM_OK;
}

// the contigs of the reference list, each once, sorted by their place in the genome
static void coverage_contigs(pssbam_engine *e) {
    e->cov_contigs.clear();
    e->cov_contigs_sent = false;
    e->cov_totals_valid = false;
    for (size_t i = 0; i < e->ref_info_host.size(); i++) {   // (the last entry answers RNAME "*": a contig of that name is listed too)
        const uint4 ri = e->ref_info_host[i];
        if (ri.w) e->cov_contigs.push_back(make_uint4(ri.x, ri.y, ri.z, (uint32_t)i));
    }
    std::stable_sort(e->cov_contigs.begin(), e->cov_contigs.end(), [](const uint4 &a, const uint4 &b) {
        return (((uint64_t)a.y << 32) | a.x) < (((uint64_t)b.y << 32) | b.x);
    });
    e->cov_contigs.erase(std::unique(e->cov_contigs.begin(), e->cov_contigs.end(), [](const uint4 &a, const uint4 &b) { return a.x == b.x && a.y == b.y; }),
                         e->cov_contigs.end());   // (a name listed twice: its first refID stands for the contig)
}

extern "C" int pssbam_engine_set_coverage(pssbam_engine *e, int32_t on, uint64_t positions_hint) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (on) {
        if (!(e->cfg.tally_mask & PSSBAM_TALLY_PSS)) return fail(PSSBAM_EINVAL, "coverage is the coverage of the reads in the substitution tables: the engine needs PSSBAM_TALLY_PSS");
        if (e->gapped) return fail(PSSBAM_EINVAL, "coverage does not go with gapped reads (pssbam_engine_set_gapped_reads): the span of a clipped or gapped read is not defined");
    }
    if (e->tallied || e->cur_feed >= 0 || !e->deferred.empty())
        return fail(PSSBAM_ESTATE, "records have been tallied already: set coverage after create or reset, before the first submit");
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t before = coverage_reserve_bytes(e);
    if (on) {
        if (e->d_genome && !e->d_cov) {   // the genome's size is known: the array now, or PSSBAM_ENOMEM
            if (const int rc = coverage_array(e, e->genome_bytes)) return rc;
            HIP_TRY(hipMemsetAsync(e->d_cov, 0, e->cov_len * sizeof(uint32_t), e->stream));
        }
        e->coverage = true;
        e->cov_hint = positions_hint;
    } else {
        e->coverage = false;
        e->cov_hint = 0;
        e->cov_win_size = 0;
        std::vector<unsigned long long>().swap(e->cov_win_sum);
        std::vector<uint32_t>().swap(e->cov_win_cov);
        std::vector<uint32_t>().swap(e->cov_win_acgt);
        std::vector<uint32_t>().swap(e->cov_win_gc);
        if (e->d_cov || e->d_cov_sums || e->d_cov_out || e->d_cov_contigs || e->d_cov_runs) {   // off: nothing stays allocated
            HIP_TRY(hipStreamSynchronize(e->stream));   // (reset's memset)
            if (e->genome_stream) HIP_TRY(hipStreamSynchronize(e->genome_stream));
            if (e->d_cov) HIP_TRY(hipFree(e->d_cov));
            if (e->d_cov_sums) HIP_TRY(hipFree(e->d_cov_sums));
            if (e->d_cov_runcnt) HIP_TRY(hipFree(e->d_cov_runcnt));
            if (e->d_cov_out) HIP_TRY(hipFree(e->d_cov_out));
            if (e->d_cov_contigs) HIP_TRY(hipFree(e->d_cov_contigs));
            if (e->d_cov_runs) HIP_TRY(hipFree(e->d_cov_runs));
            e->d_cov_runs = nullptr;
            e->cov_runs_cap = 0;
            e->cov_totals_valid = false;
            e->d_cov = nullptr;
            e->d_cov_sums = e->d_cov_runcnt = e->d_cov_out = nullptr;
            e->d_cov_contigs = nullptr;
            e->cov_len = 0;
            e->cov_sums_cap = e->cov_out_cap = e->cov_contigs_cap = 0;
            e->cov_contigs_sent = false;
        }
    }
    if (e->feed_mem_budget) {   // worked out already (pssbam_engine_feed_open): the array comes out of it, or goes back
        const uint64_t budget = e->feed_mem_budget + before, after = coverage_reserve_bytes(e);
        e->feed_mem_budget = budget > after ? budget - after : 1;
    }
    return PSSBAM_OK;
}

static uint32_t coverage_grid(const pssbam_engine *e, uint64_t n_tiles) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, (uint64_t)e->n_cu * 8));
}

// Tile sums, their scan and coverage_stats, unless the last finish's results still stand (nothing was added since): cov_out_host
// then holds the totals, d_cov_sums every tile's base and d_cov_runcnt every tile's run count.  Nothing of d_cov changes.
static int coverage_totals(pssbam_engine *e) {
    if (e->cov_totals_valid) return PSSBAM_OK;
    const uint64_t n_tiles = e->cov_len / COV_TILE;
    const size_t n_contigs = e->cov_contigs.size(), out_words = COV_OUT_CONTIGS + 3 * std::max<size_t>(n_contigs, 1);
    if (e->cov_sums_cap < n_tiles) {
        if (e->d_cov_sums) HIP_TRY(hipFree(e->d_cov_sums));
        if (e->d_cov_runcnt) HIP_TRY(hipFree(e->d_cov_runcnt));
        e->d_cov_sums = e->d_cov_runcnt = nullptr;
        e->cov_sums_cap = 0;
        if (hipMalloc((void **)&e->d_cov_sums, n_tiles * sizeof(unsigned long long)) != hipSuccess ||
            hipMalloc((void **)&e->d_cov_runcnt, n_tiles * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PSSBAM_ENOMEM, "the coverage scan's %llu tile sums do not fit the device", (unsigned long long)n_tiles);
        }
        e->cov_sums_cap = n_tiles;
    }
    if (e->cov_out_cap < out_words) {
        if (e->d_cov_out) HIP_TRY(hipFree(e->d_cov_out));
        e->d_cov_out = nullptr;
        e->cov_out_cap = 0;
        HIP_TRY(hipMalloc((void **)&e->d_cov_out, out_words * sizeof(unsigned long long)));
        e->cov_out_cap = out_words;
    }
    if (e->cov_contigs_cap < std::max<size_t>(n_contigs, 1)) {
        if (e->d_cov_contigs) HIP_TRY(hipFree(e->d_cov_contigs));
        e->d_cov_contigs = nullptr;
        e->cov_contigs_cap = 0;
        HIP_TRY(hipMalloc((void **)&e->d_cov_contigs, std::max<size_t>(n_contigs, 1) * sizeof(uint4)));
        e->cov_contigs_cap = std::max<size_t>(n_contigs, 1);
        e->cov_contigs_sent = false;
    }
    if (!e->cov_contigs_sent && n_contigs) {   // (the stream is idle: every finish drains it first)
        HIP_TRY(hipMemcpy(e->d_cov_contigs, e->cov_contigs.data(), n_contigs * sizeof(uint4), hipMemcpyHostToDevice));
        e->cov_contigs_sent = true;
    }
    HIP_TRY(hipMemsetAsync(e->d_cov_out, 0, out_words * sizeof(unsigned long long), e->stream));
    const uint32_t grid = coverage_grid(e, n_tiles);
    hipLaunchKernelGGL(coverage_tile_sums, dim3(grid), dim3(COV_THREADS), 0, e->stream, (const uint32_t *)e->d_cov, n_tiles, e->d_cov_sums);
    hipLaunchKernelGGL(coverage_scan_sums, dim3(1), dim3(COV_SUMS_ROUND), 0, e->stream, e->d_cov_sums, n_tiles, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(coverage_stats, dim3(grid), dim3(COV_THREADS), 0, e->stream, (const uint32_t *)e->d_cov, n_tiles, (const unsigned long long *)e->d_cov_sums,
                       (const uint4 *)e->d_cov_contigs, (uint32_t)n_contigs, e->d_cov_out, e->d_cov_runcnt);
    HIP_TRY(hipGetLastError());
    e->cov_out_host.assign(out_words, 0ull);
    HIP_TRY(hipMemcpyAsync(e->cov_out_host.data(), e->d_cov_out, out_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->cov_totals_valid = true;
    e->cov_runs_scanned = false;
    e->cov_epoch++;
    return PSSBAM_OK;
}

static int coverage_ready(pssbam_engine *e) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (!e->coverage) return fail(PSSBAM_EINVAL, "coverage is off (pssbam_engine_set_coverage)");
    return pssbam_engine_sync(e);
}

extern "C" int pssbam_engine_finish_coverage(pssbam_engine *e, int32_t first_ref, int32_t n, uint64_t *per_contig, uint64_t *hist, int32_t hist_max,
                                             uint64_t *n_runs) {
    int rc = coverage_ready(e);
    if (rc) return rc;
    if (hist && (hist_max < 0 || hist_max > PSSBAM_COV_HIST_MAX)) return fail(PSSBAM_EINVAL, "coverage histogram limit %d outside 0..%d", (int)hist_max, PSSBAM_COV_HIST_MAX);
    if (per_contig && (first_ref < 0 || n < 0 || (int64_t)first_ref + n > (int64_t)e->n_ref + 1))
        return fail(PSSBAM_EINVAL, "references %d..%lld outside the %d of the list (and one for \"*\")", (int)first_ref, (long long)first_ref + n, (int)e->n_ref);
    std::vector<unsigned long long> out(COV_OUT_CONTIGS + 3 * std::max<size_t>(e->cov_contigs.size(), 1), 0ull);
    if (e->d_cov && e->have_refs) {
        if ((rc = coverage_totals(e))) return rc;
        out = e->cov_out_host;
    }
    if (hist) {   // hist[d], d in 0..hist_max: positions at depth d; hist[hist_max + 1]: the positions above
        for (int32_t d = 0; d <= hist_max + 1; d++) hist[d] = 0;
        for (uint32_t d = 0; d < COV_HIST_BINS; d++) hist[std::min<uint32_t>(d, (uint32_t)hist_max + 1u)] += out[d];
    }
    if (per_contig)
        for (int32_t i = 0; i < n; i++) {
            uint64_t *o = per_contig + 3 * (size_t)i;
            o[0] = o[1] = o[2] = 0;
            const uint4 ri = e->ref_info_host[(size_t)(first_ref + i)];
            if (!ri.w) continue;   // a name the genome lacks
            const auto it = std::lower_bound(e->cov_contigs.begin(), e->cov_contigs.end(), ri, [](const uint4 &a, const uint4 &b) {
                return (((uint64_t)a.y << 32) | a.x) < (((uint64_t)b.y << 32) | b.x);
            });
            if (it == e->cov_contigs.end() || it->w != (uint32_t)(first_ref + i)) continue;   // (a name listed twice counts under its first refID)
            const size_t k = (size_t)(it - e->cov_contigs.begin());
            for (int w = 0; w < 3; w++) o[w] = out[COV_OUT_CONTIGS + 3 * k + (size_t)w];
        }
    if (n_runs) *n_runs = out[COV_OUT_RUNS];
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_coverage_runs(pssbam_engine *e, uint64_t cap, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *depth, uint64_t *n_runs) {
    int rc = coverage_ready(e);
    if (rc) return rc;
    const bool count_only = !ref && !start && !end && !depth;
    uint64_t total = 0;
    if (e->d_cov && e->have_refs) {
        if ((rc = coverage_totals(e))) return rc;
        total = e->cov_out_host[COV_OUT_RUNS];
    }
    if (n_runs) *n_runs = total;
    if (count_only) return PSSBAM_OK;
    if (cap < total) return fail(PSSBAM_EINVAL, "room for %llu runs, the coverage has %llu", (unsigned long long)cap, (unsigned long long)total);
    if (!total) return PSSBAM_OK;
    const uint64_t n_tiles = e->cov_len / COV_TILE;
    if (e->cov_runs_cap < total) {   // [slot | start | end | depth], `total` words each; kept for the next call
        if (e->d_cov_runs) HIP_TRY(hipFree(e->d_cov_runs));
        e->d_cov_runs = nullptr;
        e->cov_runs_cap = 0;
        if (hipMalloc((void **)&e->d_cov_runs, 4 * total * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PSSBAM_ENOMEM, "the %llu coverage runs do not fit the device", (unsigned long long)total);
        }
        e->cov_runs_cap = total;
    }
    uint32_t *const d_runs = e->d_cov_runs;
    std::vector<uint32_t> h(4 * total);
    if (!e->cov_runs_scanned) {
        hipLaunchKernelGGL(coverage_scan_sums, dim3(1), dim3(COV_SUMS_ROUND), 0, e->stream, e->d_cov_runcnt, n_tiles, (unsigned long long *)nullptr);
        e->cov_runs_scanned = true;
    }
    hipLaunchKernelGGL(coverage_runs, dim3(coverage_grid(e, n_tiles)), dim3(COV_THREADS), 0, e->stream, (const uint32_t *)e->d_cov, n_tiles,
                       (const unsigned long long *)e->d_cov_sums, (const unsigned long long *)e->d_cov_runcnt, (const uint4 *)e->d_cov_contigs,
                       (uint32_t)e->cov_contigs.size(), total, d_runs, d_runs + total, d_runs + 2 * total, d_runs + 3 * total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), d_runs, 4 * total * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // the device's order is the genome's (contigs by name); the caller's is by refID: a contig's runs are one stretch of it
    std::vector<std::pair<uint64_t, uint64_t>> stretch(e->cov_contigs.size(), {0, 0});
    for (uint64_t i = 0; i < total;) {
        const uint32_t s = h[i];
        uint64_t j = i + 1;
        while (j < total && h[j] == s) j++;
        if (s < stretch.size()) stretch[s] = {i, j};
        i = j;
    }
    std::vector<std::pair<uint32_t, uint32_t>> by_ref;   // {refID, slot}
    for (size_t k = 0; k < e->cov_contigs.size(); k++) by_ref.emplace_back(e->cov_contigs[k].w, (uint32_t)k);
    std::sort(by_ref.begin(), by_ref.end());
    uint64_t at = 0;
    for (const auto &rs : by_ref)
        for (uint64_t i = stretch[rs.second].first; i < stretch[rs.second].second; i++, at++) {
            if (ref) ref[at] = rs.first == (uint32_t)e->n_ref ? -1 : (int32_t)rs.first;
            if (start) start[at] = h[total + i];
            if (end) end[at] = h[2 * total + i];
            if (depth) depth[at] = h[3 * total + i];
        }
    if (at != total) return fail(PSSBAM_EHIP, "coverage runs outside the listed contigs: %llu of %llu placed", (unsigned long long)at, (unsigned long long)total);
    return PSSBAM_OK;
}

// Fixed windows over the same array (coverage_windows).  The accumulators live for the call; the result stays on the host, in genome
// order, while cov_epoch says that the totals it was computed beside still stand and the window size is the same.
extern "C" int pssbam_engine_finish_coverage_windows(pssbam_engine *e, uint32_t window, uint64_t cap, int32_t *ref, uint32_t *start, uint32_t *end,
                                                     uint32_t *acgt, uint32_t *gc, uint32_t *covered, uint64_t *depth_sum, uint64_t *n_windows) {
    int rc = coverage_ready(e);
    if (rc) return rc;
    if (window < PSSBAM_COV_WINDOW_MIN || window > PSSBAM_COV_WINDOW_MAX)
        return fail(PSSBAM_EINVAL, "window size %u outside %u..%u", window, PSSBAM_COV_WINDOW_MIN, PSSBAM_COV_WINDOW_MAX);
    if (!e->d_genome || !e->have_refs || !e->d_cov) return fail(PSSBAM_ESTATE, "windows need the genome and the references (set_genome, set_references)");
    const size_t n_contigs = e->cov_contigs.size();
    std::vector<unsigned long long> wbase(n_contigs + 1, 0ull);   // the id of each contig's first window, in genome order
    for (size_t k = 0; k < n_contigs; k++) wbase[k + 1] = wbase[k] + ((uint64_t)e->cov_contigs[k].z + window - 1) / window;
    const uint64_t total = wbase[n_contigs];
    if (total > 0xFFFFFFFFull) return fail(PSSBAM_EINVAL, "%llu windows of %u positions: the count does not fit 32 bits", (unsigned long long)total, window);
    if (n_windows) *n_windows = total;
    if (!ref && !start && !end && !acgt && !gc && !covered && !depth_sum) return PSSBAM_OK;
    if (cap < total) return fail(PSSBAM_EINVAL, "room for %llu windows, the genome has %llu", (unsigned long long)cap, (unsigned long long)total);
    if (!total) return PSSBAM_OK;
    if ((rc = coverage_totals(e))) return rc;   // the tiles' bases: those of the last finish call when nothing was added since
    if (e->cov_win_size != window || e->cov_win_epoch != e->cov_epoch || e->cov_win_sum.size() != total) {
        e->cov_win_size = 0;
        // [depth_sum | covered | acgt | gc] over the ids, then the contigs' first ids.  While windows are few the four arrays come in
        // `shards` copies (at most 1.3 MB): every workgroup at work would add to the same few words otherwise.
        const uint32_t shards = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, (1ull << 16) / total));
        const size_t cells = (size_t)total * shards;
        // the host's room first, so that nothing of the device is held when it cannot be had; one copy is read straight into it,
        // several go through h and are summed
        std::vector<unsigned long long> h;
        try {
            e->cov_win_sum.resize(total);
            e->cov_win_cov.resize(total);
            e->cov_win_acgt.resize(total);
            e->cov_win_gc.resize(total);
            if (shards > 1) h.resize(cells * (sizeof(unsigned long long) + 3 * sizeof(uint32_t)) / sizeof(unsigned long long) + 1);
        } catch (const std::bad_alloc &) {
            return fail(PSSBAM_ENOMEM, "no host memory for %llu windows", (unsigned long long)total);
        }
        const size_t acc_bytes = cells * (sizeof(unsigned long long) + 3 * sizeof(uint32_t)), wbase_bytes = std::max<size_t>(n_contigs, 1) * sizeof(unsigned long long);
        unsigned char *d_acc = nullptr;
        if (hipMalloc((void **)&d_acc, acc_bytes + wbase_bytes + 16) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PSSBAM_ENOMEM, "the accumulators of %llu windows (%llu bytes) do not fit the device", (unsigned long long)total, (unsigned long long)acc_bytes);
        }
        CovWindows W;
        W.depth_sum = (unsigned long long *)d_acc;
        W.covered = (uint32_t *)(W.depth_sum + cells);
        W.acgt = W.covered + cells;
        W.gc = W.acgt + cells;
        W.n = total;
        W.shards = shards;
        unsigned long long *const d_wbase = (unsigned long long *)(d_acc + (acc_bytes + 7) / 8 * 8);
        const uint64_t n_tiles = e->cov_len / COV_TILE;
        hipError_t err = hipMemsetAsync(d_acc, 0, acc_bytes, e->stream);
        if (err == hipSuccess && n_contigs) err = hipMemcpyAsync(d_wbase, wbase.data(), n_contigs * sizeof(unsigned long long), hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) {
            hipLaunchKernelGGL(coverage_windows, dim3(coverage_grid(e, n_tiles)), dim3(COV_THREADS), 0, e->stream, (const uint32_t *)e->d_cov,
                               (const uint8_t *)e->d_genome, e->genome_bytes, n_tiles, (const unsigned long long *)e->d_cov_sums, (const uint4 *)e->d_cov_contigs,
                               (uint32_t)n_contigs, (const unsigned long long *)d_wbase, window, W);
            err = hipGetLastError();
        }
        if (shards > 1) {
            if (err == hipSuccess) err = hipMemcpyAsync(h.data(), d_acc, acc_bytes, hipMemcpyDeviceToHost, e->stream);
        } else {
            if (err == hipSuccess) err = hipMemcpyAsync(e->cov_win_sum.data(), W.depth_sum, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream);
            if (err == hipSuccess) err = hipMemcpyAsync(e->cov_win_cov.data(), W.covered, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
            if (err == hipSuccess) err = hipMemcpyAsync(e->cov_win_acgt.data(), W.acgt, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
            if (err == hipSuccess) err = hipMemcpyAsync(e->cov_win_gc.data(), W.gc, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
        }
        const hipError_t err_sync = hipStreamSynchronize(e->stream);   // (wbase and the four vectors are read and written until here)
        (void)hipFree(d_acc);
        HIP_TRY(err);
        HIP_TRY(err_sync);
        if (shards > 1) {
            const unsigned long long *h_sum = h.data();
            const uint32_t *h_cov = (const uint32_t *)(h_sum + cells), *h_acgt = h_cov + cells, *h_gc = h_acgt + cells;
            for (uint64_t w = 0; w < total; w++) {
                unsigned long long s_sum = 0;
                uint32_t s_cov = 0, s_acgt = 0, s_gc = 0;
                for (uint32_t s = 0; s < shards; s++) {
                    s_sum += h_sum[s * total + w];
                    s_cov += h_cov[s * total + w];
                    s_acgt += h_acgt[s * total + w];
                    s_gc += h_gc[s * total + w];
                }
                e->cov_win_sum[w] = s_sum;
                e->cov_win_cov[w] = s_cov;
                e->cov_win_acgt[w] = s_acgt;
                e->cov_win_gc[w] = s_gc;
            }
        }
        e->cov_win_size = window;
        e->cov_win_epoch = e->cov_epoch;
    }
    // the device's order is the genome's (contigs by name); the caller's is by refID
    std::vector<std::pair<uint32_t, uint32_t>> by_ref;   // {refID, slot}
    for (size_t k = 0; k < n_contigs; k++) by_ref.emplace_back(e->cov_contigs[k].w, (uint32_t)k);
    std::sort(by_ref.begin(), by_ref.end());
    uint64_t at = 0;
    for (const auto &rs : by_ref) {
        const uint64_t len = e->cov_contigs[rs.second].z, first = wbase[rs.second], n = wbase[rs.second + 1] - first;
        for (uint64_t k = 0; k < n; k++, at++) {
            if (ref) ref[at] = rs.first == (uint32_t)e->n_ref ? -1 : (int32_t)rs.first;
            if (start) start[at] = (uint32_t)(k * window);
            if (end) end[at] = (uint32_t)std::min<uint64_t>((k + 1) * window, len);
            if (acgt) acgt[at] = e->cov_win_acgt[first + k];
            if (gc) gc[at] = e->cov_win_gc[first + k];
            if (covered) covered[at] = e->cov_win_cov[first + k];
            if (depth_sum) depth_sum[at] = e->cov_win_sum[first + k];
        }
    }
    return PSSBAM_OK;
}

// Duplicate flagging (dedup_kernels.h).  A filter like -R, -Q and -T, no row of the exclusive-modes table: it goes with every mode but
// gapped reads (the key of a clipped read is a question of its own).
extern "C" int pssbam_engine_set_duplicates(pssbam_engine *e, int32_t on, uint32_t initial_slots) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    if (on) {
        if (e->cfg.tally_mask != PSSBAM_TALLY_PSS && e->cfg.tally_mask != PSSBAM_TALLY_KMER)
            return fail(PSSBAM_EINVAL, "duplicates are the duplicates of one tool's candidates: PSSBAM_TALLY_PSS or PSSBAM_TALLY_KMER, not both");
        if (e->gapped) return fail(PSSBAM_EINVAL, "duplicate flagging does not go with gapped reads (pssbam_engine_set_gapped_reads): the key of a clipped read is not defined");
        if (initial_slots > DEDUP_MAX_SLOTS) return fail(PSSBAM_EINVAL, "initial_slots %u above %llu", initial_slots, (unsigned long long)DEDUP_MAX_SLOTS);
    }
    if (e->tallied || e->cur_feed >= 0 || !e->deferred.empty())
        return fail(PSSBAM_ESTATE, "records have been tallied already: set duplicate flagging after create or reset, before the first submit");
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t before = dedup_reserve_bytes(e);
    e->dedup = on != 0;
    e->dedup_initial = on ? initial_slots : 0u;
    // nothing has been inserted (create, or a reset since): the table, if there is one from an earlier run, is given back, so that
    // the next launch starts from the size asked for here, and with the setting off nothing stays allocated
    if (e->d_dedup || e->d_dedup_slot) {
        if (const int rc = dedup_poll(e, true)) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));   // (reset's dedup_clear)
        if (e->d_dedup) HIP_TRY(hipFree(e->d_dedup));
        if (e->d_dedup_slot) HIP_TRY(hipFree(e->d_dedup_slot));
        e->d_dedup = nullptr;
        e->d_dedup_slot = nullptr;
        e->dedup_cap = 0;
        e->dedup_slot_cap = 0;
    }
    if (e->feed_mem_budget) {   // worked out already (pssbam_engine_feed_open): the table comes out of it, or goes back
        const uint64_t budget = e->feed_mem_budget + before, after = dedup_reserve_bytes(e);
        e->feed_mem_budget = budget > after ? budget - after : 1;
    }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_finish_duplicates(pssbam_engine *e, uint64_t totals[3], uint64_t *hist, int32_t hist_max) {
    if (!e || !totals) return fail(PSSBAM_EINVAL, "null argument");
    if (!e->dedup) return fail(PSSBAM_EINVAL, "duplicate flagging is off (pssbam_engine_set_duplicates)");
    if (hist_max < 0 || hist_max > PSSBAM_MAX_DUP_HIST) return fail(PSSBAM_EINVAL, "duplicate histogram limit %d outside 0..%d", (int)hist_max, PSSBAM_MAX_DUP_HIST);
    int rc = pssbam_engine_sync(e);
    if (rc) return rc;
    if ((rc = dedup_poll(e, true))) return rc;
    const size_t words = 2 + (size_t)hist_max + 2;
    std::vector<unsigned long long> h(words, 0ull);
    if (e->d_dedup && e->dedup_submitted) {
        unsigned long long state = 0, *d_out = nullptr;
        HIP_TRY(hipMemcpy(&state, e->d_dedup_state, sizeof state, hipMemcpyDeviceToHost));
        if (state & DEDUP_FULL) return fail(PSSBAM_ENOMEM, "the duplicate table ran full (%llu slots): records went unflagged", (unsigned long long)e->dedup_cap);
        HIP_TRY(hipMalloc((void **)&d_out, words * sizeof(unsigned long long)));
        hipError_t q = hipMemsetAsync(d_out, 0, words * sizeof(unsigned long long), e->stream);
        if (q == hipSuccess) {
            hipLaunchKernelGGL(dedup_census, dim3(dedup_grid(e, e->dedup_cap)), dim3(256), 0, e->stream, (const DedupSlot *)e->d_dedup, e->dedup_cap, (uint32_t)hist_max, d_out);
            e->dedup_launches++;
            q = hipGetLastError();
        }
        if (q == hipSuccess) q = hipMemcpyAsync(h.data(), d_out, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream);
        if (q == hipSuccess) q = hipStreamSynchronize(e->stream);
        (void)hipFree(d_out);
        if (q != hipSuccess) return fail(PSSBAM_EHIP, "the duplicate census failed: %s", hipGetErrorString(q));
    }
    totals[0] = h[0];
    totals[1] = h[1];
    totals[2] = h[0] - h[1];
    if (hist)
        for (size_t i = 0; i < (size_t)hist_max + 2; i++) hist[i] = h[2 + i];
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_counters_device(pssbam_engine *e, void **d_counters, size_t *n_u64) {
    if (!e || !d_counters || !n_u64) return fail(PSSBAM_EINVAL, "null argument");
    *d_counters = e->d_counters;
    *n_u64 = e->n_counters;
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_genome_kmer_count(pssbam_engine *e, int klen, uint64_t *counts) {
    if (!e || !counts) return fail(PSSBAM_EINVAL, "null argument");
    if (klen < 1 || klen > PSSBAM_MAX_KLEN) return fail(PSSBAM_EINVAL, "klen %d outside the device range 1..%d", klen, PSSBAM_MAX_KLEN);
    if (!e->d_genome) return fail(PSSBAM_ESTATE, "set_genome has not been called");
    HIP_TRY(hipSetDevice(e->device));
    if (e->genome_wait_pending) {
        HIP_TRY(hipStreamWaitEvent(e->stream, e->genome_ready, 0));
        e->genome_wait_pending = false;
    }
    const size_t nb = (size_t)1 << (2 * klen);
    unsigned long long *d_bins = nullptr;
    HIP_TRY(hipMalloc(&d_bins, nb * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_bins, 0, nb * sizeof(unsigned long long), e->stream));
    hipError_t le = hipSuccess;
    if (klen <= 8 && e->d_genome4 && !getenv("PSSBAM_GKC_BYTES")) {
        // histogram in LDS from the packed genome; replication of the bins while they are few
        const uint32_t n_all = 1u << (2 * klen);
        const uint32_t n_bins = std::min<uint32_t>(n_all, 32768u);                 // per pass: <= 128 KiB of u32
        uint32_t rep_log2 = 0;
        while ((n_bins << (rep_log2 + 1)) * 4u <= 32768u && rep_log2 < 5) rep_log2++;  // up to 32 KiB of replicas
        const uint32_t lds = (n_bins << rep_log2) * 4u;
        le = hipFuncSetAttribute((const void *)genome_kmer_packed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        const uint64_t spans = (e->genome_bytes + GKC4_SPAN - 1) / GKC4_SPAN;
        const uint32_t per_cu = lds > 65536u ? 1u : 2u;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((spans + 511) / 512, (uint64_t)e->n_cu * per_cu);
        for (uint32_t lo = 0; lo < n_all && le == hipSuccess; lo += n_bins) {
            hipLaunchKernelGGL(genome_kmer_packed_kernel, dim3(blocks), dim3(512), lds, e->stream, e->d_genome4, e->genome_bytes, klen,
                               lo, n_bins, rep_log2, d_bins);
            le = hipGetLastError();
        }
    } else {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((e->genome_bytes / GKC_SPAN + 255) / 256 + 1, (uint64_t)e->n_cu * 16);
        if (klen <= 6) hipLaunchKernelGGL(genome_kmer_kernel<true>, dim3(blocks), dim3(256), 0, e->stream, e->d_genome, e->genome_bytes, klen, d_bins);
        else hipLaunchKernelGGL(genome_kmer_kernel<false>, dim3(blocks), dim3(256), 0, e->stream, e->d_genome, e->genome_bytes, klen, d_bins);
        le = hipGetLastError();
    }
    if (le == hipSuccess) le = hipMemcpyAsync(counts, d_bins, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    (void)hipFree(d_bins);
    if (le != hipSuccess) return fail(PSSBAM_EHIP, "genome k-mer count failed: %s", hipGetErrorString(le));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_bind_counters(pssbam_engine *e, void *d_counters, size_t n_u64) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    unsigned long long *target = d_counters ? (unsigned long long *)d_counters : e->d_counters_own;
    if (d_counters && (n_u64 != e->n_counters || ((uintptr_t)d_counters & 7u)))
        return fail(PSSBAM_EINVAL, "bound counter block must hold exactly %zu aligned u64 words", e->n_counters);
    if (target != e->d_counters) {
        HIP_TRY(hipMemcpyAsync(target, e->d_counters, e->n_counters * sizeof(unsigned long long),
                               hipMemcpyDeviceToDevice, e->stream));
        e->d_counters = target;
    }
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_timer_begin(pssbam_engine *e) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->t_begin, e->stream));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_timer_end(pssbam_engine *e, float *ms) {
    if (!e || !ms) return fail(PSSBAM_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->t_end, e->stream));
    HIP_TRY(hipEventSynchronize(e->t_end));
    HIP_TRY(hipEventElapsedTime(ms, e->t_begin, e->t_end));
    return PSSBAM_OK;
}

extern "C" int pssbam_engine_kernel_time(pssbam_engine *e, double *total_ms, uint64_t *n_launches, int reset) {
    if (!e) return fail(PSSBAM_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    int rc = resolve_launch_events(e);
    if (rc) return rc;
    if (total_ms) *total_ms = e->kernel_ms;
    if (n_launches) *n_launches = e->kernel_launches;
    if (reset) { e->kernel_ms = 0.0; e->kernel_launches = 0; }
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// node-level reduce (single process, several devices) over RCCL
// --------------------------------------------------------------------------------------
#include <dlfcn.h>

namespace {
// the handful of RCCL entry points used, resolved from librccl.so on first use so that
// single-GPU users never pay for loading it
typedef struct ncclComm *ncclComm_t;
typedef int (*fn_CommInitAll)(ncclComm_t *, int, const int *);
typedef int (*fn_CommDestroy)(ncclComm_t);
typedef int (*fn_GroupStart)(void);
typedef int (*fn_GroupEnd)(void);
typedef int (*fn_Reduce)(const void *, void *, size_t, int, int, int, ncclComm_t, hipStream_t);
typedef const char *(*fn_GetErrorString)(int);
constexpr int NCCL_UINT64 = 5, NCCL_SUM = 0;  // rccl.h: ncclUint64, ncclSum
struct Rccl {
    void *h = nullptr;
    fn_CommInitAll CommInitAll = nullptr;
    fn_CommDestroy CommDestroy = nullptr;
    fn_GroupStart GroupStart = nullptr;
    fn_GroupEnd GroupEnd = nullptr;
    fn_Reduce Reduce = nullptr;
    fn_GetErrorString GetErrorString = nullptr;
};
Rccl g_rccl;
bool load_rccl() {
    if (g_rccl.h) return true;
    void *h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    g_rccl.CommInitAll = (fn_CommInitAll)dlsym(h, "ncclCommInitAll");
    g_rccl.CommDestroy = (fn_CommDestroy)dlsym(h, "ncclCommDestroy");
    g_rccl.GroupStart = (fn_GroupStart)dlsym(h, "ncclGroupStart");
    g_rccl.GroupEnd = (fn_GroupEnd)dlsym(h, "ncclGroupEnd");
    g_rccl.Reduce = (fn_Reduce)dlsym(h, "ncclReduce");
    g_rccl.GetErrorString = (fn_GetErrorString)dlsym(h, "ncclGetErrorString");
    if (!g_rccl.CommInitAll || !g_rccl.CommDestroy || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.Reduce) {
        dlclose(h);
        return false;
    }
    g_rccl.h = h;
    return true;
}
}  // namespace

// One grouped ncclReduce over the engines' counter blocks (single process, one communicator per
// GPU).  PSSBAM_OK = done; 1 = RCCL is not usable here and nothing was touched (the caller sums on
// the host instead); negative = a collective failed half-way, the counters are not trustworthy.
static int reduce_rccl(pssbam_engine *const *engines, int n, int root) {
    if (!load_rccl()) return 1;
    std::vector<ncclComm_t> comms(n);
    std::vector<int> devs(n);
    for (int i = 0; i < n; i++) devs[i] = engines[i]->device;
    int rc = g_rccl.CommInitAll(comms.data(), n, devs.data());
    if (rc != 0) return 1;
    rc = g_rccl.GroupStart();
    for (int i = 0; i < n && rc == 0; i++) {
        (void)hipSetDevice(engines[i]->device);
        rc = g_rccl.Reduce(engines[i]->d_counters, engines[i]->d_counters, engines[i]->n_counters, NCCL_UINT64, NCCL_SUM,
                           root, comms[i], engines[i]->stream);
    }
    const int rc_end = g_rccl.GroupEnd();
    if (rc == 0) rc = rc_end;
    for (int i = 0; i < n; i++) {
        (void)hipSetDevice(engines[i]->device);
        (void)hipStreamSynchronize(engines[i]->stream);
    }
    for (int i = 0; i < n; i++) (void)g_rccl.CommDestroy(comms[i]);
    if (rc != 0) return fail(PSSBAM_EHIP, "ncclReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
    return PSSBAM_OK;
}

extern "C" int pssbam_reduce_counters(pssbam_engine *const *engines, int n, int root) {
    if (!engines || n < 1 || root < 0 || root >= n) return fail(PSSBAM_EINVAL, "bad argument");
    for (int i = 0; i < n; i++) {
        if (!engines[i]) return fail(PSSBAM_EINVAL, "null engine %d", i);
        if (engines[i]->n_counters != engines[0]->n_counters)
            return fail(PSSBAM_EINVAL, "engines were created with different options");
        int rc = pssbam_engine_sync(engines[i]);
        if (rc) return rc;
    }
    if (n == 1) return PSSBAM_OK;
    // RCCL needs one distinct device per rank; anything else (two engines on one GPU, librccl
    // missing, a failing communicator) takes the host-side sum below, which is also the
    // cross-check path (PSSBAM_REDUCE=host)
    bool distinct = true;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++) distinct = distinct && engines[i]->device != engines[j]->device;
    // ... and it has to be worth a communicator: ncclCommInitAll over 8 GPUs takes seconds, the pss tables are 7 KB per
    // engine (8 small copies and a host add: microseconds) -- RCCL carries the block from 32 MiB up (k-mer bins at
    // k >= 11), or when asked to (PSSBAM_REDUCE=rccl)
    const char *force = getenv("PSSBAM_REDUCE");
    const bool big = engines[0]->n_counters * sizeof(unsigned long long) >= (32ull << 20);
    if (distinct && !(force && !strcmp(force, "host")) && (big || (force && !strcmp(force, "rccl")))) {
        const int rc = reduce_rccl(engines, n, root);
        if (rc <= 0) return rc;
    }

    const size_t nc = engines[0]->n_counters;
    std::vector<unsigned long long> sum(nc, 0ull), part(nc);
    for (int i = 0; i < n; i++) {
        HIP_TRY(hipSetDevice(engines[i]->device));
        HIP_TRY(hipMemcpy(part.data(), engines[i]->d_counters, nc * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nc; k++) sum[k] += part[k];
    }
    HIP_TRY(hipSetDevice(engines[root]->device));
    HIP_TRY(hipMemcpy(engines[root]->d_counters, sum.data(), nc * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return PSSBAM_OK;
}

extern "C" int pssbam_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(PSSBAM_EINVAL, "bad argument");
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return PSSBAM_OK;
}

extern "C" int pssbam_host_unregister(void *ptr) {
    if (!ptr) return fail(PSSBAM_EINVAL, "bad argument");
    HIP_TRY(hipHostUnregister(ptr));
    return PSSBAM_OK;
}

// --------------------------------------------------------------------------------------
// host helper: record index
// --------------------------------------------------------------------------------------
extern "C" int64_t pssbam_index_records(const void *bytes, uint64_t nbytes, uint32_t *offsets, uint64_t max_records,
                                        uint64_t *consumed) {
    const uint8_t *p = (const uint8_t *)bytes;
    uint64_t o = 0, n = 0;
    while (n < max_records && o + 4 <= nbytes && o < (1ull << 32) - 4) {
        uint32_t bs;
        memcpy(&bs, p + o, 4);
        if (bs < 32) { fail(PSSBAM_EFORMAT, "record %llu: block_size %u < 32", (unsigned long long)n, bs); return PSSBAM_EFORMAT; }
        const uint64_t next = o + 4 + (uint64_t)bs;
        if (next > nbytes || next >= (1ull << 32)) break;  // partial record: caller supplies more bytes
        if (offsets) offsets[n] = (uint32_t)o;
        n++;
        o = next;
    }
    if (offsets) offsets[n] = (uint32_t)o;
    if (consumed) *consumed = o;
    return (int64_t)n;
}

// --------------------------------------------------------------------------------------
// device-side BGZF inflate
// --------------------------------------------------------------------------------------
#include "bgzf_api.h"
