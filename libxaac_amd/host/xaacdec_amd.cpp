/*
 * xaacdec_amd.cpp -- the native command line decoder of this repo: ADTS AAC-LC / HE-AAC / HE-AACv2 in, 16-bit WAV out, as
 * `xaacdec` (test/decoder/ixheaacd_main.c over decoder/ixheaacd_api.c:2624-3788) decodes it -- with the reference's default
 * -esbr:1 (SBR streams through the float eSBR tools, "Path A") or with -esbr:0 (the fixed-point SBR tools) -- with the repo's own
 * host front end (include/xaac_parse.h, CPU threads) in front of the GPU entry points of include/xaac_amd.h and every
 * stream's state resident in device memory.  No reference code, no Python, no torch: HIP runtime + the two libraries.
 *
 *   xaacdec_amd -ifile:<in.aac> -ofile:<out.wav> [-esbr:<0|1>] [-copies:<N>] [-verify] [-threads:<T>] [-quiet]
 *   xaacdec_amd -ilist:<file with one input path per line> -odir:<directory> [-esbr:<0|1>] [-threads:<T>] [-serialgroups:<0|1>] [-quiet]
 *   ... [-gpus:<G>] [-device:<k>] [-plan] [-gputools:<0|1>] [-mcsbr:<0|1>]
 *   ... [-downmix:<0|1>] [-dmix:<0|1>] [-tostereo:<0|1>] [-peak_limiter_off:<0|1>]
 *   ... [-drc_cut_fac:<0..1>] [-drc_boost_fac:<0..1>] [-drc_target_level:<0..127>]
 * Any of the three -drc_* flags switches MPEG-4 dynamic range control on, as in the reference (api.c:1927-1946): the
 * dynamic_range_info of an AAC-LC stream's fill elements is decoded by the front end, its gain factors go up beside the spectra and
 * xaac_drc_apply_batch multiplies them in front of the IMDCT (behind the -gputools:1 stage); the limiter runs behind as before.
 * Flags not given keep the reference's cut 1, boost 1, target level 108.  In a mixed list they act on the AAC-LC groups.  Refused
 * before a device is looked at or a file written: with an SBR stream in the list, with more than two channels, -drc_heavy_comp:1,
 * values out of range.
 *
 * The reference's output stage flags, on the GPU (include/xaac_amd.h: xaac_out_map; the mapped calls store the mapped block only, and
 * the device PCM buffers, the copy down, the pinned staging and -verify all have the mapped channel count):
 *   -downmix:1           a stream of 3 .. 6 channels comes out in stereo (ixheaacd_dec_downmix_to_stereo); refused for one or two channels
 *   -dmix:1              a stereo AAC-LC stream comes out mono ((l >> 1) + (r >> 1)), with -tostereo:1 that word twice; a no-op on a mono
 *                        AAC-LC stream; refused with SBR, with more than two channels, with -downmix:1
 *   -tostereo:1          a mono AAC-LC stream comes out with its channel twice; a no-op on everything else
 *   -peak_limiter_off:1  AAC-LC: ixheaacd_scale_adjust + round16 in the limiter's place; a no-op with SBR (no limiter on that path)
 * -tostereo:1, -peak_limiter_off:1 and the no-op cases write the reference's bytes.  -downmix:1 and -dmix:1 write a file that is right
 * where the reference's is not: a 44-byte PCM header with the mapped channel count and every sample of the unflagged decode mixed --
 * the reference's header keeps the stream's channel count over stereo data and its tail (the limiter's flushed delay line) is unmixed.
 *
 * -mcsbr:1 (default 0) takes HE-AAC streams of more than two channels (channel_config 3 .. 6 with SBR payloads): one SBR decoder per
 * channel element, as the reference keeps them; default flags (-esbr:1) only.  Without the flag such a stream is refused.
 *
 * -gputools:1 (default 0) runs the M/S, intensity, PNS and TNS tools on the GPU: the streams are parsed up to the entry of
 * ixheaacd_channel_pair_process (stage 1), the tools' side rows go up beside the spectra and xaac_aac_tools_process_batch runs in
 * front of the IMDCT.  The output is the same; without the flag nothing of that path is allocated or launched.
 *
 * -gpus:G shards the batch's streams over G devices of this node (k, k + 1, ... from -device:k, default 0): contiguous ranges
 * whose sizes differ by at most one -- libxaac_amd/dist.py: shard_range, the split bench.py --gpus N makes over ranks -- one host
 * thread, HIP context, stream and set of resident states per device, nothing shared between the shards but the read-only
 * inputs (streams are independent: no data-path exchange; the PCM of every shard comes down to its own host thread).
 * -plan prints the split and exits before anything touches a device (tests/test_cli_plan_cpu.py); -wrap_devices lets the
 * shards wrap around the devices the node has (two shards on one device: the -gpus host path on a one-GPU box, tests/test_cli_gpu.py).
 *
 * -copies:N decodes N instances of the stream in one lock-step batch (the first one's PCM is written; with -verify all N are
 * compared with it word for word) and prints the end-to-end rate: the shape a serving host has, with one input here for brevity.
 * -ilist decodes different streams in one run, each to <odir>/<name>.wav.  The streams of one kind (core sampling rate, one or two
 * channels, an SBR payload in the first frame or not) are a group, in list order: one lock-step batch with its own Job, in which a
 * stream that ends drops out of the steps and the others go on.  A list of several kinds has several groups, and every (device,
 * group) that has streams gets a host thread with its own HIP stream and context, as the shards of -gpus do: the groups run side by
 * side and share only the parser library's team (-threads:T is divided over them in proportion to their streams).  Every flag
 * means for a group what it means for a list of that kind alone; an output stage flag that one group refuses refuses the run, with
 * the first such file's name, before a device is looked at.  Every file has its own group's channels, rate and header; the closing
 * line's "groups" array (only there for several groups) has the groups in the order of their first files.  -serialgroups:1 runs
 * the groups one after the other (the same files: to measure what side by side gains, or to find the group that fails).  A stream
 * of more than two channels is only taken beside streams of its own kind: mixed with others the list is refused up front.
 *
 * The shape of a shard (decode_shard), the same as libxaac_amd/decoder.py has in Python (used by the tests for its ease of
 * inspection): ShardOwner hands out and releases what the shard allocates; ParseSide owns the parsers, the staging groups and
 * the helper thread; ShardDriver owns what every kind of stream shares and runs the step loop; ToolsStage is -gputools:1; the
 * chain picked once -- LcChain, SbrChain (-esbr:0) or EsbrChain (Path A, over a QmfTransposer or a DftTransposer) -- owns its
 * streams' device-resident states.  A new kind of stream is a new Chain.
 */
#include <hip/hip_runtime_api.h>
#include <ctype.h>
#include <sched.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xaac_amd.h"
#include "../../include/xaac_esbr.h"
#include "../../include/xaac_parse.h"

namespace {

/* a combination of flags and stream this decoder does not take: its own message, no output file */
[[noreturn]] void reject(const char *why) {
  fprintf(stderr, "xaacdec_amd: %s\n", why);
  exit(2);
}
[[noreturn]] void die(const char *what, long code = 0) {
  fprintf(stderr, "xaacdec_amd: %s failed (%ld)\n", what, code);
  exit(2);
}
#define HIP(x)                         \
  do {                                 \
    hipError_t e_ = (x);               \
    if (e_ != hipSuccess) die(#x, e_); \
  } while (0)
#define XA(x)                 \
  do {                        \
    int32_t e_ = (x);         \
    if (e_ != 0) die(#x, e_); \
  } while (0)

/* CPUs of the NUMA node the GPU hangs off (hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<id>/numa_node -> the node's
   cpulist); an empty set where that cannot be read.  Pinned staging memory is allocated and first touched from there:
   with the staging on the other socket the bus carries one direction at full rate but both at once -- spectra going up
   beside the PCM of the step before coming down -- at 38 GiB/s in total instead of 63 (a two-socket MI355X host). */
cpu_set_t gpu_node_cpus(int device, bool *known) {
  cpu_set_t set;
  CPU_ZERO(&set);
  *known = false;
  char id[64] = {0}, path[160];
  if (hipDeviceGetPCIBusId(id, (int)sizeof(id), device) != hipSuccess) return set;
  for (char *c = id; *c; c++) *c = (char)tolower(*c);
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", id);
  int node = -1;
  if (FILE *f = fopen(path, "r")) {
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
  }
  if (node < 0) return set;
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen(path, "r");
  if (!f) return set;
  int a, b;
  for (;;) {
    if (fscanf(f, "%d", &a) != 1) break;
    b = a;
    int ch = fgetc(f);
    if (ch == '-') {
      if (fscanf(f, "%d", &b) != 1) break;
      ch = fgetc(f);
    }
    for (int c = a; c <= b && c < CPU_SETSIZE; c++) CPU_SET(c, &set), *known = true;
    if (ch != ',') break;
  }
  fclose(f);
  return set;
}
/* the GPU's NUMA node is looked up once per device (the shards of a -gpus run sit on different nodes of a two-socket host) */
cpu_set_t near_cpus(int device, bool *known) { /* (by value: the table may grow under another shard's thread) */
  static std::mutex mu;
  static std::vector<std::pair<int, std::pair<bool, cpu_set_t>>> seen;
  std::lock_guard<std::mutex> lk(mu);
  for (auto &e : seen)
    if (e.first == device) return *known = e.second.first, e.second.second;
  bool k = false;
  const cpu_set_t set = gpu_node_cpus(device, &k);
  seen.push_back({device, {k, set}});
  *known = k;
  return seen.back().second.second;
}

/* What one shard allocates and makes, and the one place where all of it goes again: zeroed device arrays, pinned arrays near
   the GPU, the HIP streams and events, the xaac_ctx and the parsers.  The destructor waits for the streams and then releases
   everything, so a shard's share of a -gpus run does not stay behind until the process ends.  (die() exits the process
   without unwinding: nothing is released on that path, and nothing has to be.) */
class ShardOwner {
 public:
  explicit ShardOwner(int device) : device_(device) { HIP(hipSetDevice(device)); }
  ShardOwner(const ShardOwner &) = delete;
  ~ShardOwner() {
    (void)hipSetDevice(device_); /* (main's thread releases the shards) */
    for (hipStream_t s : streams_) (void)hipStreamSynchronize(s);
    for (void *p : dev_) (void)hipFree(p);
    for (void *p : host_) (void)hipHostFree(p);
    for (xaac_parser *p : parsers_) xaac_parser_destroy(p);
    if (ctx_) (void)xaac_destroy(ctx_);
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
    for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
  }
  hipStream_t stream() {
    hipStream_t s;
    HIP(hipStreamCreate(&s));
    streams_.push_back(s);
    return s;
  }
  hipEvent_t event() {
    hipEvent_t e;
    HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    events_.push_back(e);
    return e;
  }
  xaac_ctx *context(hipStream_t s) {
    XA(xaac_create(&ctx_, device_, s));
    return ctx_;
  }
  xaac_parser *parser() {
    xaac_parser *p = nullptr;
    XA(xaac_parser_create(&p));
    parsers_.push_back(p);
    return p;
  }
  void *workspace(uint64_t bytes) { /* device bytes as they come: the kernels that take a workspace write it before they read it */
    void *p = nullptr;
    HIP(hipMalloc(&p, bytes ? bytes : 16));
    dev_.push_back(p);
    return p;
  }
  template <class T>
  T *dev(size_t n) {
    void *p = workspace(n * sizeof(T));
    HIP(hipMemset(p, 0, n * sizeof(T) ? n * sizeof(T) : 16));
    return static_cast<T *>(p);
  }
  template <class T>
  T *pinned(size_t n) {
    bool known = false;
    const cpu_set_t near = near_cpus(device_, &known);
    cpu_set_t before, both;
    /* first touch on the GPU's NUMA node: only CPUs this thread may run on anyway (a cpuset that does not meet the node leaves the
       thread where it is) */
    bool moved = false;
    if (known && sched_getaffinity(0, sizeof(before), &before) == 0) {
      CPU_AND(&both, &before, &near);
      moved = CPU_COUNT(&both) > 0 && sched_setaffinity(0, sizeof(both), &both) == 0;
    }
    void *p = nullptr;
    HIP(hipHostMalloc(&p, n * sizeof(T) ? n * sizeof(T) : 16, hipHostMallocDefault));
    host_.push_back(p);
    memset(p, 0, n * sizeof(T) ? n * sizeof(T) : 16);
    if (moved) sched_setaffinity(0, sizeof(before), &before);
    return static_cast<T *>(p);
  }

 private:
  const int device_;
  std::vector<void *> dev_, host_;
  std::vector<hipStream_t> streams_;
  std::vector<hipEvent_t> events_;
  std::vector<xaac_parser *> parsers_;
  xaac_ctx *ctx_ = nullptr;
};

struct Staging { /* what one step's parse leaves for the GPU */
  int32_t *spec;
  uint8_t *ics;
  xaac_sbr_header *header;
  xaac_sbr_frame *frame;
  xaac_ps_frame *ps;
  xaac_esbr_side *eside;
  xaac_core_tools_side *tside; /* -gputools:1: the side info of the M/S, intensity, PNS and TNS tools */
  xaac_drc_side *dside;        /* -drc_*: a row of band ends and gain factors beside every row of spec */
  const int32_t *flags, *status, *reset_pitch; /* the step's rows of its group's vectors: [N][XAAC_SBR_FLAG_WORDS], [N], [N] */
  int delivered;
  int lines; /* leading spectral lines that may be non-zero in a delivered row (xaac_parse_batch::lines, rounded up to 64) */
};

/* what one parser call fills: kFramesPerParse steps, their pinned arrays one behind the other (xaac_parse_batch::frames) */
constexpr int kFramesPerParse = 4;
struct StagingGroup {
  std::vector<int32_t> flags, status, reset_pitch, lines;
  std::vector<uint64_t> consumed;
};

/* More than two channels: the reference's WAVE_FORMAT_EXTENSIBLE header (test/decoder/ixheaacd_main.c: a 40-byte fmt chunk with the
   channel mask of ixheaacd_get_channel_mask and the PCM sub-format GUID; its RIFF size counts 36 bytes in front of the data as
   for the plain header), 68 bytes in front of the samples */
void write_wav_extensible(FILE *f, size_t samples, int channels, int rate, uint32_t mask) {
  const uint32_t data = (uint32_t)(samples * 2), riff = 36 + data, fmt = 40, byte_rate = (uint32_t)(rate * channels * 2), sr = (uint32_t)rate;
  const uint16_t tag = 0xfffe, ch = (uint16_t)channels, align = (uint16_t)(channels * 2), bits = 16, cb = 22;
  static const uint8_t pcm_guid[16] = {0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71};
  fwrite("RIFF", 1, 4, f), fwrite(&riff, 4, 1, f), fwrite("WAVEfmt ", 1, 8, f), fwrite(&fmt, 4, 1, f);
  fwrite(&tag, 2, 1, f), fwrite(&ch, 2, 1, f), fwrite(&sr, 4, 1, f), fwrite(&byte_rate, 4, 1, f);
  fwrite(&align, 2, 1, f), fwrite(&bits, 2, 1, f), fwrite(&cb, 2, 1, f), fwrite(&bits, 2, 1, f), fwrite(&mask, 4, 1, f);
  fwrite(pcm_guid, 1, 16, f), fwrite("data", 1, 4, f), fwrite(&data, 4, 1, f);
}

void write_wav(const std::string &path, const std::vector<int16_t> &pcm, int channels, int rate, uint32_t mask = 0) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) die("fopen(output)");
  if (channels > 2) {
    write_wav_extensible(f, pcm.size(), channels, rate, mask);
    fwrite(pcm.data(), 2, pcm.size(), f);
    fclose(f);
    return;
  }
  const uint32_t data = (uint32_t)(pcm.size() * 2), riff = 36 + data, fmt = 16, byte_rate = (uint32_t)(rate * channels * 2);
  const uint16_t pcm_tag = 1, ch = (uint16_t)channels, align = (uint16_t)(channels * 2), bits = 16;
  const uint32_t sr = (uint32_t)rate;
  fwrite("RIFF", 1, 4, f), fwrite(&riff, 4, 1, f), fwrite("WAVEfmt ", 1, 8, f), fwrite(&fmt, 4, 1, f);
  fwrite(&pcm_tag, 2, 1, f), fwrite(&ch, 2, 1, f), fwrite(&sr, 4, 1, f), fwrite(&byte_rate, 4, 1, f);
  fwrite(&align, 2, 1, f), fwrite(&bits, 2, 1, f), fwrite("data", 1, 4, f), fwrite(&data, 4, 1, f);
  fwrite(pcm.data(), 2, pcm.size(), f);
  fclose(f);
}

/* what the command line fixes for every shard of one group: the streams of one kind (core sampling rate, channels, SBR or not) of
   a list in list order, or the copies of the one input */
struct Job {
  std::vector<std::vector<uint8_t>> datas; /* -ilist: one per stream of the group; else the one input */
  std::vector<int> index;                  /* -ilist: where each of them stands in the list (what the messages call it) */
  int n_ch, sbr, esbr, out_ch, rate, per;
  int channel_config; /* 3 .. 6: a stream of several channel elements (with sbr: -mcsbr:1, Path A only); 0: one element, the mono / stereo paths */
  int n_els;          /* channel elements of a frame: 1, or the configuration's 2 .. 4 */
  int first_ch[4];    /* ... and the first bitstream channel of each */
  int slot[8];        /* ... output channel of bitstream channel c: where the reference routes its elements (layout_of) */
  int el_of_ch[8];    /* ... channel element of bitstream channel c */
  /* the row of a step's flag / reset pitch vectors that covers channel row i of the shard: per stream, or -- more than two channels
     with SBR -- per channel element of the stream (xaac_parse_batch::mc_sbr) */
  size_t flag_row(int i) const { return channel_config && sbr ? (size_t)(i / n_ch) * n_els + el_of_ch[i % n_ch] : (size_t)(i / n_ch); }
  /* such a stream's rows stay in bitstream order on the device (the hand-off behind the SBR calls routes them); an AAC-LC one's
     are routed on their way up */
  bool routed_up() const { return channel_config && !sbr; }
  int hq; /* -esbr_hq:1: the DFT harmonic transposer in the QMF one's place (Path A only) */
  int threads, verify, profile;
  int gputools; /* -gputools:1: parse at stage 1, the spectral tools run on the GPU in front of the IMDCT */
  xaac_out_map map; /* -downmix:1 / -dmix:1 / -tostereo:1: what the PCM hand-off does to a sample's channels (out_ch is the mapped count) */
  int lim_off;      /* -peak_limiter_off:1 on an AAC-LC stream */
  int drc;          /* a -drc_* flag on an AAC-LC stream: dynamic range control in front of the IMDCT, with ... */
  xaac_drc_config drc_cfg;
  bool list_mode;
};
/* one device's share of the batch: streams [lo, lo + n) on HIP device `device`, decoded by one host thread */
struct Shard {
  int device, lo, n;
  std::vector<std::vector<int16_t>> pcms; /* every stream's output (-ilist), or the shard's first stream's */
  long frames = 0, mismatched = 0, first_frames = 0;
  double parse_s = 0, wall = 0, steady = 0, phase_s[4] = {0, 0, 0, 0};
  std::unique_ptr<ShardOwner> mem; /* what the shard allocated, until main lets go of it */
};

/* libxaac_amd/dist.py: shard_range -- contiguous [lo, hi) of n items owned by shard r of g; sizes differ by at most one */
void shard_range(int n, int r, int g, int *lo, int *hi) {
  const int base = n / g, rem = n % g;
  *lo = r * base + (r < rem ? r : rem);
  *hi = *lo + base + (r < rem ? 1 : 0);
}

/* what a chain wants staged beside the spectra and the window info */
struct Wants {
  bool sbr, ps, esbr; /* SBR headers and frames; PS frames; the eSBR side rows (and parsers that read them) */
};

/* The parse side of a shard: the streams' parsers and read positions, three groups of kFramesPerParse staging sets and the
   helper thread that fills them.  It knows nothing of what runs on the GPU.
   Three groups of kFramesPerParse steps: the parse of group g + 1 | the copies up and kernels of group g's steps | the copy
   down of the step before.  A stream's parser state and bytes are fetched once per call for kFramesPerParse frames (on the
   2 x 64-core box 32 threads parse 3.9-4.6 x 10^6 frames/s one frame per call, 4.9-5.6 x 10^6 with 2..8).  A step's flag,
   status and pitch rows are its group's: they stay as parsed until the group is parsed again, two groups of steps later, and
   the step's PCM is consumed one step late. */
class ParseSide {
 public:
  static constexpr int T = kFramesPerParse;
  ParseSide(const Job &J, Shard &S, ShardOwner &mem, Wants w)
      : J_(J), N_(S.n), lo_(S.lo), parse_s_(S.parse_s), parser_((size_t)S.n), ptr_((size_t)S.n), left_((size_t)S.n), pos_((size_t)S.n, 0),
        broken_((size_t)S.n, 0) {
    const int N = N_, NC = N * J.n_ch;
    for (auto &p : parser_) {
      p = mem.parser();
      if (w.esbr) XA(xaac_parser_set_esbr(p, 1));
      if (J.drc) XA(xaac_parse_drc_config(p, &J.drc_cfg));
    }
    for (int g = 0; g < 3; g++) {
      int32_t *spec = mem.pinned<int32_t>((size_t)T * NC * 1024);
      uint8_t *ics = mem.pinned<uint8_t>((size_t)T * NC * 2);
      xaac_sbr_header *header = w.sbr ? mem.pinned<xaac_sbr_header>((size_t)T * NC) : nullptr;
      xaac_sbr_frame *frame = w.sbr ? mem.pinned<xaac_sbr_frame>((size_t)T * NC) : nullptr;
      xaac_ps_frame *psf = w.ps ? mem.pinned<xaac_ps_frame>((size_t)T * N) : nullptr;
      xaac_esbr_side *eside = w.esbr ? mem.pinned<xaac_esbr_side>((size_t)T * NC) : nullptr;
      const int NE = J.n_els; /* the tools' side rows: one per channel element, element-major within a step */
      xaac_core_tools_side *tside = J.gputools ? mem.pinned<xaac_core_tools_side>((size_t)T * N * NE) : nullptr;
      xaac_drc_side *dside = J.drc ? mem.pinned<xaac_drc_side>((size_t)T * NC) : nullptr;
      StagingGroup &G = grp_[g];
      const int NF = J.channel_config && J.sbr ? NE : 1; /* flag rows of a stream: one, or one per channel element (mc_sbr) */
      G.flags.assign((size_t)T * N * NF * XAAC_SBR_FLAG_WORDS, 0), G.status.assign((size_t)T * N, 0), G.reset_pitch.assign((size_t)T * N * NF, 0);
      G.lines.assign((size_t)T * N, 0), G.consumed.assign((size_t)N, 0);
      for (int t = 0; t < T; t++) {
        Staging &s = st_[g * T + t];
        s.spec = spec + (size_t)t * NC * 1024, s.ics = ics + (size_t)t * NC * 2;
        s.header = header ? header + (size_t)t * NC : nullptr, s.frame = frame ? frame + (size_t)t * NC : nullptr;
        s.ps = psf ? psf + (size_t)t * N : nullptr, s.eside = eside ? eside + (size_t)t * NC : nullptr;
        s.tside = tside ? tside + (size_t)t * N * NE : nullptr;
        s.dside = dside ? dside + (size_t)t * NC : nullptr;
        s.flags = &G.flags[(size_t)t * N * NF * XAAC_SBR_FLAG_WORDS], s.status = &G.status[(size_t)t * N], s.reset_pitch = &G.reset_pitch[(size_t)t * N * NF];
        s.delivered = 0, s.lines = 1024;
      }
    }
    for (int i = 0; i < N; i++) {
      const std::vector<uint8_t> &d = J.datas[J.list_mode ? (size_t)(lo_ + i) : 0];
      ptr_[(size_t)i] = d.data(), left_[(size_t)i] = d.size(); /* the whole streams: the library keeps the read positions (pos) */
    }
    /* one helper thread for the whole run: it parses the next staging set when told to, the main thread waits for `done` */
    worker_ = std::thread([this] { work(); });
  }
  ~ParseSide() { stop(); }
  void start() { /* the next group's frames are parsed from here on */
    std::lock_guard<std::mutex> lk(mu_);
    job_++;
    cv_.notify_all();
  }
  void wait(int group) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return done_ >= group; });
  }
  void stop() {
    if (!worker_.joinable()) return;
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
      cv_.notify_all();
    }
    worker_.join();
  }
  const Staging &step(int which) const { return st_[which]; }
  xaac_parser *const *parsers() const { return parser_.data(); }

 private:
  void work() {
    for (int expect = 0;; expect++) {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return quit_ || job_ > expect; });
      if (quit_) return;
      lk.unlock();
      parse(expect % 3);
      lk.lock();
      done_ = expect;
      cv_.notify_all();
    }
  }
  void parse(int g) { /* the next kFramesPerParse frames of every stream into one group of staging sets */
    const auto t0 = std::chrono::steady_clock::now();
    const int N = N_;
    StagingGroup &G = grp_[g];
    for (int i = 0; i < N; i++)
      if (broken_[(size_t)i]) left_[(size_t)i] = 0;
    xaac_parse_batch b;
    memset(&b, 0, sizeof(b));
    b.n_streams = N, b.n_ch = J_.n_ch, b.with_sbr = J_.sbr, b.ps_enable = 1, b.stage = J_.gputools ? 1 : 2, b.threads = J_.threads;
    b.channel_config = J_.channel_config, b.mc_sbr = J_.channel_config && J_.sbr;
    b.parser = parser_.data(), b.data = ptr_.data(), b.bytes = left_.data(), b.pos = pos_.data(), b.frames = T;
    Staging &s0 = st_[g * T];
    b.spec = s0.spec, b.ics = s0.ics, b.header = s0.header, b.frame = s0.frame, b.ps_frame = s0.ps;
    b.flags = G.flags.data(), b.consumed = G.consumed.data(), b.status = G.status.data(), b.esbr_side = s0.eside;
    b.reset_pitch = G.reset_pitch.data(), b.lines = G.lines.data(), b.tools_side = s0.tside;
    b.drc_side = s0.dside;
    const int ok = xaac_parse_batch_run(&b);
    if (ok < 0) die("xaac_parse_batch_run", ok);
    for (int t = 0; t < T; t++) {
      Staging &s = st_[g * T + t];
      int delivered = 0, lines = 0;
      for (int i = 0; i < N; i++) {
        int32_t &r = G.status[(size_t)t * N + i];
        if (r < 0) {
          /* one file of a list with trailing bytes or damage must not take the other streams' output along: that stream ends
             here (what it delivered so far is written), the batch goes on */
          if (!J_.list_mode) die("a frame does not parse", r);
          if (!broken_[(size_t)i])
            fprintf(stderr, "xaacdec_amd: stream %d: a frame does not parse (%d) at byte %llu: the stream ends here\n", J_.index[(size_t)(lo_ + i)], r,
                    (unsigned long long)pos_[(size_t)i]);
          broken_[(size_t)i] = 1;
          r = XAAC_PARSE_NEED_DATA;
        }
        if (r == 0) {
          delivered++;
          lines = G.lines[(size_t)t * N + i] > lines ? G.lines[(size_t)t * N + i] : lines;
        }
      }
      s.delivered = delivered;
      s.lines = (lines + 63) & ~63;
    }
    parse_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

  const Job &J_;
  const int N_, lo_;
  double &parse_s_;
  std::vector<xaac_parser *> parser_;
  std::vector<const uint8_t *> ptr_;
  std::vector<uint64_t> left_, pos_;
  std::vector<char> broken_; /* -ilist: a stream whose frame did not parse is treated as over from there on */
  Staging st_[3 * T];
  StagingGroup grp_[3];
  std::mutex mu_;
  std::condition_variable cv_;
  int job_ = 0, done_ = -1;
  bool quit_ = false;
  std::thread worker_;
};

/* what the driver shows a chain or a stage: the shard's shape, its owner, the context and stream, and the per-step buffers
   that are the same for every kind of stream */
struct Env {
  const Job &J;
  int N, NC;
  ShardOwner &mem;
  xaac_ctx *ctx;
  hipStream_t stream;
  int32_t *d_spec;
  int16_t *d_pcm[2];    /* PCM of a step, one per slot */
  int32_t *d_status[2]; /* [NC] status words of a step's SBR kernels, one per slot */
  xaac_imdct_batch imdct; /* the IMDCT over d_spec / d_ics / d_overlap / d_ovl; a chain adds where its output goes */
};

/* what the driver has to know of a step to bring its PCM down */
struct StepOut {
  const int16_t *d_pcm;
  size_t bytes;
  bool mono_twice; /* [N][2048] mono samples came down: the host doubles them to stereo */
  bool some_mono;  /* a PS batch with streams that have no PS in this frame: their left samples also go to the right */
  int status_rows; /* rows of the slot's d_status the step's kernels wrote (n_ch per stream), 0: none */
};

/* One kind of stream's work between the copies up and the copy down, with the device-resident states and buffers it needs:
   picked once per shard.  A new kind of stream is a class with these members. */
class Chain {
 public:
  virtual ~Chain() {}
  virtual Wants wants() const = 0;
  virtual StepOut run(const Staging &s, int slot) = 0; /* the step's own copies up and its kernels, on the shard's stream */
  virtual void stream_ended(int) {}                    /* -ilist: stream i delivered its last frame in the step before */
  virtual size_t first_frame_skip() const { return 0; }     /* int16 words cut from the front of every stream's first frame */
  virtual bool drops_first_frame() const { return false; }  /* the first frame is decoded but not written */
  virtual void finish(std::vector<std::vector<int16_t>> &) {} /* what the chain still holds of every stream's output */
};

/* -gputools:1: the tools' side rows, the streams' noise generators (begin() gives them what a new stream's start from), the
   kernel's status words; the driver runs this in front of whichever chain */
class ToolsStage {
 public:
  explicit ToolsStage(const Env &E) : E_(E), rows_((size_t)E.N * E.J.n_els) {
    d_side_ = E.mem.dev<xaac_core_tools_side>(rows_), d_state_ = E.mem.dev<xaac_core_tools_state>(rows_);
    HIP(hipMemset(d_state_, 0, rows_ * sizeof(xaac_core_tools_state)));
    for (int k = 0; k < 2; k++) d_status_[k] = E.mem.dev<int32_t>(rows_), h_status_[k] = E.mem.pinned<int32_t>(rows_);
  }
  /* behind the parse of the streams' first frames, in front of the first run: every element's generator as its stage-1 parser
     says a new stream's starts (xaac_parse_core_tools_state_mc; a stream without a first frame keeps zeros) */
  void begin(xaac_parser *const *parser) {
    std::vector<xaac_core_tools_state> h(rows_);
    memset(static_cast<void *>(h.data()), 0, rows_ * sizeof(xaac_core_tools_state));
    for (int k = 0; k < E_.J.n_els; k++)
      for (int i = 0; i < E_.N; i++) xaac_parse_core_tools_state_mc(parser[i], k, &h[(size_t)k * E_.N + i]);
    HIP(hipMemcpyAsync(d_state_, h.data(), rows_ * sizeof(xaac_core_tools_state), hipMemcpyHostToDevice, E_.stream));
    HIP(hipStreamSynchronize(E_.stream));
  }
  void send_up(const Staging &s) {
    HIP(hipMemcpyAsync(d_side_, s.tside, rows_ * sizeof(xaac_core_tools_side), hipMemcpyHostToDevice, E_.stream));
  }
  /* stage-1 spectra -> the spectra the IMDCT takes, in place (xaac_parse_batch::lines covers what they reach).  Side, state and
     status rows are element-major: one launch per element index over all streams, from the element's first channel row (a pair's
     channels are neighbouring rows in the output order too), the stream's rows apart */
  void run(int slot) {
    const size_t N = (size_t)E_.N;
    for (int k = 0; k < E_.J.n_els; k++) {
      xaac_aac_tools_batch tb;
      memset(&tb, 0, sizeof(tb));
      const int row = E_.J.routed_up() ? E_.J.slot[E_.J.first_ch[k]] : E_.J.first_ch[k];
      tb.n = E_.N, tb.spec_stride = 1024 * E_.J.n_ch, tb.spec = E_.d_spec + (size_t)row * 1024;
      tb.side = d_side_ + k * N, tb.state = d_state_ + k * N, tb.status = d_status_[slot] + k * N;
      XA(xaac_aac_tools_process_batch(E_.ctx, &tb));
    }
  }
  void bring_down(int slot, hipStream_t down) {
    HIP(hipMemcpyAsync(h_status_[slot], d_status_[slot], rows_ * 4, hipMemcpyDeviceToHost, down));
  }
  const int32_t *status(int slot) const { return h_status_[slot]; } /* [n_els][N] */

 private:
  const Env E_;
  const size_t rows_;
  xaac_core_tools_side *d_side_;
  xaac_core_tools_state *d_state_;
  int32_t *d_status_[2], *h_status_[2];
};

/* AAC-LC: IMDCT -> limiter -> round16 (api.c:3662-3692) */
class LcChain : public Chain {
 public:
  explicit LcChain(const Env &E) : E_(E) {
    const int N = E.N, n_ch = E.J.n_ch;
    d_out32_ = E.mem.dev<int32_t>((size_t)N * 1024 * n_ch);
    d_qadj_ = E.mem.dev<int8_t>((size_t)N * n_ch);
    d_lim_ = E.mem.dev<xaac_limiter_state>((size_t)N);
    xaac_limiter_state l0;
    delay_ = xaac_peak_limiter_init(&l0, (uint32_t)n_ch, (uint32_t)E.J.rate);
    if (delay_ < 0) die("xaac_peak_limiter_init", delay_);
    for (int i = 0; i < N; i++) HIP(hipMemcpy(d_lim_ + i, &l0, sizeof(l0), hipMemcpyHostToDevice));
    ws_bytes_ = xaac_peak_limiter_workspace_bytes(N);
    d_ws_ = E.mem.workspace(ws_bytes_);
    kept_.assign((size_t)N, 0);
    if (E.J.list_mode) lim_at_end_.resize((size_t)N);
    mapped_ = E.J.map.kind != XAAC_OUT_MAP_NONE;
    d_dside_ = E.J.drc ? E.mem.dev<xaac_drc_side>((size_t)E.NC) : nullptr;
  }
  Wants wants() const override { return {false, false, false}; }
  StepOut run(const Staging &s, int slot) override {
    const int N = E_.N, n_ch = E_.J.n_ch;
    if (E_.J.drc) { /* ixheaacd_drc_apply in front of ixheaacd_imdct_process (aacdecoder.c:981-992): the step's rows, then the launch */
      HIP(hipMemcpyAsync(d_dside_, s.dside, (size_t)E_.NC * sizeof(xaac_drc_side), hipMemcpyHostToDevice, E_.stream));
      xaac_drc_batch db;
      memset(&db, 0, sizeof(db));
      db.n = E_.NC, db.spec_stride = 1024, db.spec = E_.d_spec, db.side = d_dside_;
      XA(xaac_drc_apply_batch(E_.ctx, &db));
    }
    xaac_imdct_batch ib = E_.imdct;
    const bool planar = E_.imdct.ch_fac == 1 && n_ch > 1; /* more than two channels: the IMDCT writes [stream][channel][1024] */
    const size_t bytes = (size_t)N * E_.J.per * E_.J.out_ch * 2;
    if (E_.J.lim_off && !mapped_ && n_ch <= 2) { /* -peak_limiter_off:1: the IMDCT's own hand-off (XAAC_PCM_LC: scale_adjust + round16) */
      ib.pcm16 = E_.d_pcm[slot], ib.pcm_mode = XAAC_PCM_LC;
      XA(xaac_imdct_process_batch(E_.ctx, &ib));
      return {E_.d_pcm[slot], bytes, false, false, 0};
    }
    ib.out32 = d_out32_, ib.qshift_adj = d_qadj_;
    XA(xaac_imdct_process_batch(E_.ctx, &ib));
    if (E_.J.lim_off) { /* ... for more channels, or with a map: a sample's channels meet in one lane behind the IMDCT */
      xaac_scale_adjust_map_batch sb;
      memset(&sb, 0, sizeof(sb));
      sb.n_streams = N, sb.frame_len = 1024, sb.num_channels = n_ch, sb.planar = planar, sb.samples = d_out32_, sb.stride = 1024 * n_ch;
      sb.qshift_adj = d_qadj_, sb.pcm16 = E_.d_pcm[slot], sb.map = E_.J.map;
      XA(xaac_pcm16_scale_adjust_map_batch(E_.ctx, &sb));
      return {E_.d_pcm[slot], bytes, false, false, 0};
    }
    xaac_limiter_batch lb;
    memset(&lb, 0, sizeof(lb));
    lb.n_streams = N, lb.frame_len = 1024, lb.samples = d_out32_, lb.stride = 1024 * n_ch, lb.qshift_adj = d_qadj_, lb.state = d_lim_;
    lb.num_channels = n_ch, lb.pcm16 = E_.d_pcm[slot], lb.workspace = d_ws_, lb.workspace_bytes = ws_bytes_;
    lb.planar = planar;
    if (mapped_) { /* the map is the limiter's epilogue: only the mapped block is stored */
      xaac_limiter_map_batch mb;
      mb.lim = lb, mb.map = E_.J.map;
      XA(xaac_peak_limiter_process_map_batch(E_.ctx, &mb));
    } else {
      XA(xaac_peak_limiter_process_batch(E_.ctx, &lb));
    }
    return {E_.d_pcm[slot], bytes, false, false, 0};
  }
  void stream_ended(int i) override { /* the limiter state a stream leaves behind its last frame */
    if (E_.J.lim_off) return;
    HIP(hipMemcpy(&lim_at_end_[(size_t)i], d_lim_ + i, sizeof(xaac_limiter_state), hipMemcpyDeviceToHost)); /* (waits for the step before) */
    kept_[(size_t)i] = 1;
  }
  size_t first_frame_skip() const override { return (size_t)delay_ * E_.J.out_ch; } /* the limiter's delay is cut from the first frame */
  void finish(std::vector<std::vector<int16_t>> &pcms) override {
    /* the limiter's delay line holds the last attack_time_samples samples: api.c:2824-2866 */
    const int n_ch = E_.J.n_ch;
    static thread_local xaac_limiter_state l;
    std::vector<int16_t> tail;
    for (size_t i = 0; i < pcms.size(); i++) {
      if (E_.J.lim_off) { /* -peak_limiter_off:1: the reference flushes the delay line all the same, and nothing ever went into it */
        pcms[i].insert(pcms[i].end(), (size_t)delay_ * E_.J.out_ch, (int16_t)0);
        continue;
      }
      if (kept_[i]) l = lim_at_end_[i];
      else HIP(hipMemcpy(&l, d_lim_ + i, sizeof(l), hipMemcpyDeviceToHost));
      const uint32_t att = l.attack_time_samples, at = l.delayed_input_index;
      tail.clear();
      for (uint32_t k = 0; k < att; k++)
        for (int c = 0; c < n_ch; c++) {
          const float v = l.delayed_input[(size_t)((at + k) % att) * n_ch + c];
          const int64_t w = (v >= 2147483648.0f || v < -2147483648.0f || v != v) ? INT32_MIN : (int64_t)v; /* (WORD32)v as x86 has it */
          int64_t r = w + 0x8000;
          if (r > INT32_MAX) r = INT32_MAX;
          tail.push_back((int16_t)(r >> 16));
        }
      /* the flushed samples take the map the frames took, on the host (the CPU twin of the mapped calls), in place: a mono
         channel written twice needs the room of two */
      tail.resize((size_t)att * (size_t)(n_ch > E_.J.out_ch ? n_ch : E_.J.out_ch));
      const int32_t oc = xaac_out_map_apply_host(&E_.J.map, n_ch, tail.data(), (int64_t)att, tail.data());
      if (oc != E_.J.out_ch) die("xaac_out_map_apply_host", oc);
      pcms[i].insert(pcms[i].end(), tail.begin(), tail.begin() + (size_t)att * oc);
    }
  }

 private:
  const Env E_;
  int32_t *d_out32_;
  int8_t *d_qadj_;
  xaac_limiter_state *d_lim_;
  xaac_drc_side *d_dside_; /* -drc_*: the step's rows on the device */
  void *d_ws_;
  uint64_t ws_bytes_;
  int delay_;
  std::vector<xaac_limiter_state> lim_at_end_; /* -ilist: the limiter state a stream leaves behind its last frame */
  std::vector<char> kept_;
  bool mapped_ = false;
};

/* -esbr:0, the fixed-point SBR tools: IMDCT -> low-power SBR for pairs, HQ SBR + parametric stereo for mono streams */
class SbrChain : public Chain {
 public:
  explicit SbrChain(const Env &E) : E_(E), mono_(E.J.n_ch == 1) {
    const int N = E.N, NC = E.NC;
    d_core_ = E.mem.dev<int16_t>((size_t)NC * 1024);
    d_header_ = E.mem.dev<xaac_sbr_header>((size_t)NC);
    d_frame_ = E.mem.dev<xaac_sbr_frame>((size_t)NC);
    d_state_ = E.mem.dev<xaac_sbr_state>((size_t)NC);
    xaac_sbr_state s0;
    xaac_sbr_state_init(&s0);
    {
      std::vector<xaac_sbr_state> all((size_t)NC, s0);
      HIP(hipMemcpy(d_state_, all.data(), all.size() * sizeof(s0), hipMemcpyHostToDevice));
    }
    d_flags_ = E.mem.dev<int32_t>((size_t)N * XAAC_SBR_FLAG_WORDS), h_flags_ = E.mem.pinned<int32_t>((size_t)N * XAAC_SBR_FLAG_WORDS);
    if (mono_) {
      d_psf_ = E.mem.dev<xaac_ps_frame>((size_t)N);
      d_ps_state_ = E.mem.dev<xaac_ps_state>((size_t)N);
      d_mono_[0] = E.mem.dev<int16_t>((size_t)N * 2048), d_mono_[1] = E.mem.dev<int16_t>((size_t)N * 2048);
      d_idx_ = E.mem.dev<int32_t>((size_t)N);
      xaac_ps_state p0;
      xaac_ps_state_init(&p0);
      {
        std::vector<xaac_ps_state> all((size_t)N, p0);
        HIP(hipMemcpy(d_ps_state_, all.data(), all.size() * sizeof(p0), hipMemcpyHostToDevice));
      }
      ws_bytes_ = xaac_sbr_hq_workspace_bytes(N, 1);
    } else {
      ws_bytes_ = xaac_sbr_lp_workspace_bytes(NC);
    }
    d_ws_ = E.mem.workspace(ws_bytes_);
  }
  Wants wants() const override { return {true, mono_, false}; }
  StepOut run(const Staging &s, int slot) override {
    xaac_imdct_batch ib = E_.imdct;
    ib.pcm16 = d_core_, ib.pcm_mode = XAAC_PCM_SBR;
    XA(xaac_imdct_process_batch(E_.ctx, &ib));
    HIP(hipMemcpyAsync(d_header_, s.header, (size_t)E_.NC * sizeof(xaac_sbr_header), hipMemcpyHostToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_frame_, s.frame, (size_t)E_.NC * sizeof(xaac_sbr_frame), hipMemcpyHostToDevice, E_.stream));
    apply_side(s);
    return mono_ ? run_hq_ps(s, slot) : run_lp(slot);
  }

 private:
  /* frames that reset the SBR decoder or fall back to plain up-sampling rewrite a few words of the resident state: on
     the device, from the flag rows (a stream that is over keeps its last frame's flags: its row goes up as zeros) */
  void apply_side(const Staging &s) {
    const int N = E_.N;
    bool any = false;
    for (int i = 0; i < N; i++) {
      const int32_t *f = &s.flags[(size_t)i * XAAC_SBR_FLAG_WORDS];
      any = any || (s.status[(size_t)i] == 0 && (f[XAAC_SBR_FLAG_RESET] || f[XAAC_SBR_FLAG_UPSAMPLING]));
    }
    if (!any) return;
    /* h_flags is one pinned buffer: an earlier step's copy up may still be reading it, so the stream is drained BEFORE the
       rows are rewritten (rewriting first and draining behind, as this did, could hand that copy the new rows) */
    HIP(hipStreamSynchronize(E_.stream));
    for (int i = 0; i < N; i++) {
      const int32_t *f = &s.flags[(size_t)i * XAAC_SBR_FLAG_WORDS];
      const bool live = s.status[(size_t)i] == 0;
      for (int k = 0; k < XAAC_SBR_FLAG_WORDS; k++) h_flags_[(size_t)i * XAAC_SBR_FLAG_WORDS + k] = live ? f[k] : 0;
    }
    HIP(hipMemcpyAsync(d_flags_, h_flags_, (size_t)N * XAAC_SBR_FLAG_WORDS * sizeof(int32_t), hipMemcpyHostToDevice, E_.stream));
    xaac_sbr_apply_side_batch ab;
    memset(&ab, 0, sizeof(ab));
    ab.n_streams = N, ab.ch_fac = E_.J.n_ch, ab.header = d_header_, ab.flags = d_flags_, ab.state = d_state_;
    ab.ps_state = mono_ ? d_ps_state_ : nullptr;
    XA(xaac_sbr_state_apply_side_batch(E_.ctx, &ab));
  }
  StepOut run_lp(int slot) {
    xaac_sbr_lp_batch b;
    memset(&b, 0, sizeof(b));
    b.n_ch = E_.NC, b.in_ch_fac = 2, b.out_ch_fac = 2, b.pcm_in = d_core_, b.header = d_header_, b.frame = d_frame_;
    b.state = d_state_, b.pcm_out = E_.d_pcm[slot], b.status = E_.d_status[slot], b.workspace = d_ws_, b.workspace_bytes = ws_bytes_;
    XA(xaac_sbr_lp_process_batch(E_.ctx, &b));
    return {E_.d_pcm[slot], (size_t)E_.N * E_.J.per * E_.J.out_ch * 2, false, false, E_.NC};
  }
  StepOut run_hq_ps(const Staging &s, int slot) {
    const int N = E_.N;
    int with_ps = 0, starts = 0;
    std::vector<int32_t> idx;
    for (int i = 0; i < N; i++) {
      with_ps += s.status[(size_t)i] == 0 && s.flags[(size_t)i * XAAC_SBR_FLAG_WORDS + XAAC_SBR_FLAG_PS] != 0;
      if (s.status[(size_t)i] == 0 && s.flags[(size_t)i * XAAC_SBR_FLAG_WORDS + XAAC_SBR_FLAG_PS_START]) idx.push_back(i), starts++;
    }
    /* streams with and without parametric stereo in one step (independent HE-AAC / HE-AACv2 streams, or streams whose PS
       starts at different frames): the batch runs with the PS launch, which passes a stream without PS through as the mono
       frame it is (sbr_ps_kernel.hip: sbr_dec.c:1246) -- its right bank stays idle, its left samples are doubled on the host */
    const bool some_mono = with_ps != 0 && with_ps != s.delivered;
    xaac_sbr_hq_batch b;
    memset(&b, 0, sizeof(b));
    b.n_ch = N, b.in_ch_fac = 1, b.out_ch_fac = 1, b.pcm_in = d_core_, b.header = d_header_, b.frame = d_frame_;
    b.state = d_state_, b.status = E_.d_status[slot], b.workspace = d_ws_, b.workspace_bytes = ws_bytes_;
    if (with_ps) {
      if (starts) { /* the right bank starts from the left one's filter states (sbrdecoder.c:762-775) */
        HIP(hipMemcpyAsync(d_idx_, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, E_.stream));
        HIP(hipStreamSynchronize(E_.stream));
        xaac_sbr_handover_batch hb;
        memset(&hb, 0, sizeof(hb));
        hb.n = starts, hb.mode = XAAC_HANDOVER_PS_START, hb.src = d_idx_, hb.dst = d_idx_, hb.state = d_state_, hb.ps_state = d_ps_state_;
        XA(xaac_sbr_state_handover(E_.ctx, &hb));
      }
      HIP(hipMemcpyAsync(d_psf_, s.ps, (size_t)N * sizeof(xaac_ps_frame), hipMemcpyHostToDevice, E_.stream));
      b.ps_frame = d_psf_, b.ps_state = d_ps_state_, b.pcm_out = E_.d_pcm[slot];
    } else {
      b.pcm_out = d_mono_[slot];
    }
    XA(xaac_sbr_hq_process_batch(E_.ctx, &b));
    if (!with_ps) return {d_mono_[slot], (size_t)N * 2048 * 2, true, some_mono, E_.NC};
    return {E_.d_pcm[slot], (size_t)N * E_.J.per * E_.J.out_ch * 2, false, some_mono, E_.NC};
  }

  const Env E_;
  const bool mono_;
  int16_t *d_core_, *d_mono_[2] = {nullptr, nullptr};
  xaac_sbr_header *d_header_;
  xaac_sbr_frame *d_frame_;
  xaac_sbr_state *d_state_;
  xaac_ps_frame *d_psf_ = nullptr;
  xaac_ps_state *d_ps_state_ = nullptr;
  int32_t *d_idx_ = nullptr;
  int32_t *d_flags_, *h_flags_; /* the parser's flag rows as xaac_sbr_state_apply_side_batch takes them */
  void *d_ws_;
  uint64_t ws_bytes_;
};

/* The channels one reset of the SBR decoder covers, and with that how their rows move between the channels' places and the
   scratch planes of the reset-time transposer runs: every channel of the shard with a constant number of strided 2-D copies
   (every stream's first frame: the whole batch), or the listed channels gathered into the first slots of the planes. */
struct ResetSet {
  bool gathered;
  std::vector<int> chs; /* gathered: the channels, slot k of the planes holds channel chs[k] */
  int n;                /* channels in the runs */
  int units() const { return gathered ? n : 1; } /* a gathered channel each, or all channels at once */
};
struct RowMove {
  float *scratch; /* in slot 0's plane */
  void *home;     /* channel 0's rows; channel i's are `pitch` bytes times i further on */
  size_t pitch;
  int rows;
};
/* the scratch of the reset-time runs: [NC][32][64] planes of the transposer's input and output rows, and a word per channel */
struct ResetScratch {
  float *q_re, *q_im, *pv_re, *pv_im;
  int32_t *idx;
};

/* Which harmonic transposer Path A runs with: what it keeps per channel, how a reset re-initialises it, its two reset-time
   runs, and what it adds to a frame's batch. */
class Transposer {
 public:
  virtual ~Transposer() {}
  virtual bool always_gathers() const = 0; /* no strided form: a whole-batch reset gathers every channel */
  virtual bool ph_rows_in() const = 0;     /* the second run's output rows 24..31 start from the state's ph rows */
  virtual void new_parameters(const Staging &s, const ResetSet &R) = 0; /* host work in front of the drain */
  virtual void stage(const Staging &s, const ResetSet &R, const ResetScratch &sc, int u) = 0; /* unit u's states made ready for the runs */
  virtual void upload(const ResetSet &R, const ResetScratch &sc) = 0;   /* the runs' per-channel words */
  virtual void run(const ResetSet &R, const ResetScratch &sc, int32_t *d_status) = 0;
  virtual void back(const ResetSet &R, int u) = 0; /* unit u's states to their places */
  virtual void attach(xaac_esbr_sbr_batch &b, const Staging &s) = 0;
};

/* the QMF transposer (the reference's default) */
class QmfTransposer : public Transposer {
 public:
  explicit QmfTransposer(const Env &E) : E_(E) { d_hbe_ = E.mem.dev<xaac_hbe_state>((size_t)E.NC); /* all zero for a new stream */ }
  bool always_gathers() const override { return false; }
  bool ph_rows_in() const override { return true; }
  /* the transposer's parameters from the new band tables (its two delay lines cleared, hbe_trans.c:102-222) */
  void new_parameters(const Staging &s, const ResetSet &R) override {
    static thread_local xaac_hbe_state h0;
    if (tail_.empty()) tail_.assign((size_t)E_.NC * kTail, 0);
    if (R.gathered && !d_tmp_) d_tmp_ = E_.mem.dev<xaac_hbe_state>((size_t)E_.NC);
    pitch_.resize((size_t)R.n);
    for (int k = 0; k < R.n; k++) {
      const int i = R.gathered ? R.chs[(size_t)k] : k;
      xaac_hbe_state_init(&h0);
      memcpy(&h0.synth_size, &tail_[(size_t)i * kTail], kTail);
      if (xaac_hbe_state_reinit(&h0, &s.header[(size_t)i])) die("the QMF transposer refused the SBR band tables");
      memcpy(&tail_[(size_t)i * kTail], &h0.synth_size, kTail);
      pitch_[(size_t)k] = s.reset_pitch[E_.J.flag_row(i)];
    }
  }
  void stage(const Staging &, const ResetSet &R, const ResetScratch &sc, int u) override {
    constexpr size_t kSynth = sizeof(xaac_hbe_state::synth_buf), kAnaly = sizeof(xaac_hbe_state::analy_buf);
    if (R.gathered) { /* the channel's state into d_tmp_: new parameters from the band tables, delay lines cleared */
      const int i = R.chs[(size_t)u];
      HIP(hipMemcpyAsync(&d_tmp_[u], &d_hbe_[i], sizeof(xaac_hbe_state), hipMemcpyDeviceToDevice, E_.stream));
      HIP(hipMemcpyAsync(&d_tmp_[u].synth_size, &tail_[(size_t)i * kTail], kTail, hipMemcpyHostToDevice, E_.stream));
      HIP(hipMemsetAsync(&d_tmp_[u].synth_buf[0], 0, kSynth, E_.stream));
      HIP(hipMemsetAsync(&d_tmp_[u].analy_buf[0], 0, kAnaly, E_.stream));
    } else {
      HIP(hipMemcpy2D(&d_hbe_[0].synth_size, sizeof(xaac_hbe_state), tail_.data(), kTail, kTail, (size_t)E_.NC, hipMemcpyHostToDevice));
      HIP(hipMemset2DAsync(&d_hbe_[0].synth_buf[0], sizeof(xaac_hbe_state), 0, kSynth, (size_t)E_.NC, E_.stream));
      HIP(hipMemset2DAsync(&d_hbe_[0].analy_buf[0], sizeof(xaac_hbe_state), 0, kAnaly, (size_t)E_.NC, E_.stream));
      HIP(hipMemcpy(sc.idx, pitch_.data(), (size_t)R.n * 4, hipMemcpyHostToDevice));
    }
  }
  void upload(const ResetSet &R, const ResetScratch &sc) override {
    if (!R.gathered) return; /* (they went up with the states, by a copy that returns when it is done) */
    HIP(hipMemcpyAsync(sc.idx, pitch_.data(), (size_t)R.n * 4, hipMemcpyHostToDevice, E_.stream));
    HIP(hipStreamSynchronize(E_.stream)); /* (pitch and the tails are host memory of this scope) */
  }
  void run(const ResetSet &R, const ResetScratch &sc, int32_t *d_status) override {
    xaac_hbe_apply_batch_desc hb;
    memset(&hb, 0, sizeof(hb));
    hb.n_ch = R.n, hb.qmf_re = sc.q_re, hb.qmf_im = sc.q_im, hb.state = R.gathered ? d_tmp_ : d_hbe_, hb.pv_re = sc.pv_re, hb.pv_im = sc.pv_im;
    hb.status = d_status, hb.pitch_in_bins = sc.idx;
    hb.max_synth_size = hint();
    XA(xaac_hbe_apply_batch(E_.ctx, &hb));
  }
  void back(const ResetSet &R, int u) override {
    if (R.gathered) HIP(hipMemcpyAsync(&d_hbe_[R.chs[(size_t)u]], &d_tmp_[u], sizeof(xaac_hbe_state), hipMemcpyDeviceToDevice, E_.stream));
  }
  void attach(xaac_esbr_sbr_batch &b, const Staging &) override {
    b.hbe_state = d_hbe_;
    b.hbe_max_synth_size = hint();
  }

 private:
  static constexpr size_t kTail = sizeof(xaac_hbe_state) - offsetof(xaac_hbe_state, synth_size); /* the integers behind the buffers */
  int32_t hint() const { /* the largest bank of the batch, as the ABI's LDS hint takes it: 8, or 0 = any */
    int32_t smax = 0, v;
    for (size_t i = 0; i * kTail < tail_.size(); i++) memcpy(&v, &tail_[i * kTail], 4), smax = v > smax ? v : smax;
    return smax <= 8 ? 8 : 0;
  }
  const Env E_;
  xaac_hbe_state *d_hbe_, *d_tmp_ = nullptr; /* d_tmp_: the resetting channels of a step gathered (partial resets) */
  std::vector<uint8_t> tail_; /* every channel's transposer integers, kept between resets: some survive one (max_stretch, fft_ready) */
  std::vector<int32_t> pitch_;
};

/* -esbr_hq:1: every channel's DFT transposer, the configurations their headers' band tables gave (shared by channels with the
   same tables), and what the host keeps between resets: max_stretch (the re-initialisation leaves it alone when four patches
   fit), the last processed frame's over_sampling_flag (the reset-time runs use the transposer's: sbr_dec.c:884 sets it) */
class DftTransposer : public Transposer {
 public:
  explicit DftTransposer(const Env &E) : E_(E) {
    const size_t NC = (size_t)E.NC;
    d_dft_ = E.mem.dev<xaac_hbe_dft_state>(NC); /* all zero for a new stream: refused (last_status -1) until a header sets it up */
    d_tmp_ = E.mem.dev<xaac_hbe_dft_state>(NC);
    d_cfg_ = E.mem.dev<xaac_hbe_dft_cfg>(NC);
    d_coef_ = E.mem.dev<float>(2 * NC * 64 * 128);
    d_slot_ = E.mem.dev<int32_t>(NC), d_slot_tmp_ = E.mem.dev<int32_t>(NC), d_ovs_ = E.mem.dev<int32_t>(NC);
    ms_.assign(NC, 0), ovs_.assign(NC, 0), slot_.assign(NC, 0);
  }
  bool always_gathers() const override { return true; }
  bool ph_rows_in() const override { return false; } /* its output rows are written whole (rows32) */
  void new_parameters(const Staging &, const ResetSet &R) override {
    r_pitch_.resize((size_t)R.n), r_slot_.resize((size_t)R.n), r_ovs_.resize((size_t)R.n);
  }
  /* ixheaacd_dft_hbe_data_reinit on the host (xaac_hbe_dft_state_reinit: sizes, windows, matrices; a configuration is shared
     by the channels whose band tables are the same), the channel's state into d_tmp_ */
  void stage(const Staging &s, const ResetSet &R, const ResetScratch &, int u) override {
    static thread_local xaac_hbe_dft_state h0;
    static thread_local xaac_hbe_dft_cfg c0;
    static thread_local float k_re[64 * 128], k_im[64 * 128];
    constexpr size_t kInts = sizeof(xaac_hbe_dft_state) - offsetof(xaac_hbe_dft_state, anal.analy_size); /* the integers behind the signals */
    const int i = R.chs[(size_t)u], NC = E_.NC;
    const xaac_sbr_header &hd = s.header[(size_t)i];
    memset(&h0, 0, sizeof(h0));
    h0.max_stretch = ms_[(size_t)i];
    if (xaac_hbe_dft_state_reinit(&h0, &c0, k_re, k_im, &hd)) die("the DFT transposer has no windows for the SBR band tables");
    ms_[(size_t)i] = h0.max_stretch;
    const std::string key(reinterpret_cast<const char *>(&hd.num_sf_bands[0]),
                          reinterpret_cast<const char *>(&hd.freq_band_tbl_noise[0]) - reinterpret_cast<const char *>(&hd.num_sf_bands[0]));
    const std::string key2 = key + std::string(reinterpret_cast<const char *>(&h0.max_stretch), 4);
    auto it = cfgs_.find(key2);
    if (it == cfgs_.end()) { /* a configuration no channel of the shard has had yet: its windows and matrices go up (synchronously: host temporaries) */
      const int slot = (int)cfgs_.size();
      if (slot >= NC) die("more DFT transposer configurations than channels");
      it = cfgs_.emplace(key2, slot).first;
      HIP(hipMemcpy(&d_cfg_[slot], &c0, sizeof(c0), hipMemcpyHostToDevice));
      HIP(hipMemcpy(d_coef_ + (size_t)slot * 64 * 128, k_re, sizeof(k_re), hipMemcpyHostToDevice));
      HIP(hipMemcpy(d_coef_ + ((size_t)NC + slot) * 64 * 128, k_im, sizeof(k_im), hipMemcpyHostToDevice));
    }
    slot_[(size_t)i] = r_slot_[(size_t)u] = it->second;
    HIP(hipMemcpy(&d_dft_[i].anal.analy_size, &h0.anal.analy_size, kInts, hipMemcpyHostToDevice));
    HIP(hipMemset(&d_dft_[i].synth_buf[0], 0, sizeof(h0.synth_buf))); /* hbe_dft_trans.c:302 */
    HIP(hipMemcpyAsync(&d_tmp_[u], &d_dft_[i], sizeof(xaac_hbe_dft_state), hipMemcpyDeviceToDevice, E_.stream));
    r_pitch_[(size_t)u] = s.reset_pitch[E_.J.flag_row(i)];
    r_ovs_[(size_t)u] = ovs_[(size_t)i];
  }
  void upload(const ResetSet &R, const ResetScratch &sc) override {
    HIP(hipMemcpyAsync(sc.idx, r_pitch_.data(), (size_t)R.n * 4, hipMemcpyHostToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_slot_tmp_, r_slot_.data(), (size_t)R.n * 4, hipMemcpyHostToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_ovs_, r_ovs_.data(), (size_t)R.n * 4, hipMemcpyHostToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_slot_, slot_.data(), (size_t)E_.NC * 4, hipMemcpyHostToDevice, E_.stream));
    HIP(hipStreamSynchronize(E_.stream)); /* (the vectors are host memory of this scope) */
  }
  void run(const ResetSet &R, const ResetScratch &sc, int32_t *d_status) override {
    xaac_hbe_dft_apply_batch db;
    memset(&db, 0, sizeof(db));
    db.n_ch = R.n, db.qmf_re = sc.q_re, db.qmf_im = sc.q_im, db.pitch_in_bins = sc.idx, db.oversampling = d_ovs_, db.cfg_tab = d_cfg_;
    db.coef_re = d_coef_, db.coef_im = d_coef_ + (size_t)E_.NC * 64 * 128, db.cfg = d_slot_tmp_, db.state = d_tmp_;
    db.pv_re = sc.pv_re, db.pv_im = sc.pv_im, db.status = d_status, db.rows32 = 1;
    XA(xaac_hbe_dft_apply_batch_run(E_.ctx, &db));
  }
  void back(const ResetSet &R, int u) override {
    HIP(hipMemcpyAsync(&d_dft_[R.chs[(size_t)u]], &d_tmp_[u], sizeof(xaac_hbe_dft_state), hipMemcpyDeviceToDevice, E_.stream));
  }
  void attach(xaac_esbr_sbr_batch &b, const Staging &s) override {
    b.hbe_dft_state = d_dft_, b.hbe_dft_cfg_tab = d_cfg_, b.hbe_dft_cfg = d_slot_;
    b.hbe_dft_coef_re = d_coef_, b.hbe_dft_coef_im = d_coef_ + (size_t)E_.NC * 64 * 128;
    for (int i = 0; i < E_.NC; i++) /* the flag the transposer keeps for a reset that may follow */
      if (s.status[(size_t)(i / E_.J.n_ch)] == 0 && s.frame[(size_t)i].apply_processing)
        ovs_[(size_t)i] = (s.eside[(size_t)i].harmonic_sbr & XAAC_ESBR_OVERSAMPLING) ? 1 : 0;
  }

 private:
  const Env E_;
  xaac_hbe_dft_state *d_dft_, *d_tmp_;
  xaac_hbe_dft_cfg *d_cfg_;
  float *d_coef_;                            /* [2][NC][64][128]: real matrices of the configurations, then the imaginary ones */
  int32_t *d_slot_, *d_slot_tmp_, *d_ovs_;   /* [NC] configuration of a channel; of the gathered channels; their flags */
  std::vector<int32_t> ms_, ovs_, slot_;     /* per channel: max_stretch, over_sampling_flag, configuration */
  std::vector<int32_t> r_pitch_, r_slot_, r_ovs_; /* per gathered channel of the reset at hand */
  std::map<std::string, int> cfgs_;
};

/* -esbr:1, Path A: IMDCT -> float planes -> eSBR chain (+ transposer, float PS) -> samples_sat */
class EsbrChain : public Chain {
 public:
  explicit EsbrChain(const Env &E) : E_(E), mono_(E.J.n_ch == 1), mc_(E.J.channel_config != 0) {
    const int N = E.N, NC = E.NC;
    if (mc_) d_out32_ = E.mem.dev<int32_t>((size_t)NC * 1024), d_qadj_ = E.mem.dev<int8_t>((size_t)NC);
    else d_core_ = E.mem.dev<int16_t>((size_t)NC * 1024);
    d_header_ = E.mem.dev<xaac_sbr_header>((size_t)NC);
    d_frame_ = E.mem.dev<xaac_sbr_frame>((size_t)NC);
    d_eside_ = E.mem.dev<xaac_esbr_side>((size_t)NC);
    d_estate_ = E.mem.dev<xaac_esbr_state>((size_t)NC);
    if (E.J.hq) tr_.reset(new DftTransposer(E));
    else tr_.reset(new QmfTransposer(E));
    d_fcore_ = E.mem.dev<float>((size_t)NC * 1024);
    d_out_l_ = E.mem.dev<float>((size_t)NC * 2048);
    d_older_ = E.mem.dev<float>((size_t)2 * NC * 24 * 64);
    static thread_local xaac_esbr_state e0; /* (thread_local: one shard per device thread) */
    xaac_esbr_state_init(&e0);
    for (int i = 0; i < NC; i++) HIP(hipMemcpy(d_estate_ + i, &e0, sizeof(e0), hipMemcpyHostToDevice));
    if (mono_) {
      d_psf_ = E.mem.dev<xaac_ps_frame>((size_t)N);
      d_eps_ = E.mem.dev<xaac_esbr_ps_state>((size_t)N);
      d_out_r_ = E.mem.dev<float>((size_t)N * 2048);
      static thread_local xaac_esbr_ps_state p0;
      xaac_esbr_ps_state_init(&p0);
      for (int i = 0; i < N; i++) HIP(hipMemcpy(d_eps_ + i, &p0, sizeof(p0), hipMemcpyHostToDevice));
    }
    ws_bytes_ = xaac_esbr_workspace_bytes(NC);
    d_ws_ = E.mem.workspace(ws_bytes_);
  }
  Wants wants() const override { return {true, mono_, true}; }
  /* (with -esbr:1 the reference's command line decoder does not write an SBR stream's first frame:
     test/decoder/ixheaacd_main.c:2181-2186) */
  bool drops_first_frame() const override { return true; }
  StepOut run(const Staging &s, int slot) override {
    const int N = E_.N, NC = E_.NC;
    xaac_imdct_batch ib = E_.imdct;
    if (mc_) ib.out32 = d_out32_, ib.qshift_adj = d_qadj_; /* every channel a row (ch_fac 1): the hand-in below converts them */
    else ib.pcm16 = d_core_, ib.pcm_mode = XAAC_PCM_SBR;
    XA(xaac_imdct_process_batch(E_.ctx, &ib));
    int resets = 0, with_ps = 0; /* channel rows that reset; streams with PS (never with more than two channels) */
    for (int i = 0; i < NC; i++)
      if (s.status[(size_t)(i / E_.J.n_ch)] == 0) resets += s.flags[E_.J.flag_row(i) * XAAC_SBR_FLAG_WORDS + XAAC_SBR_FLAG_RESET] != 0;
    for (int i = 0; i < N && !mc_; i++)
      if (s.status[(size_t)i] == 0) with_ps += s.flags[(size_t)i * XAAC_SBR_FLAG_WORDS + XAAC_SBR_FLAG_PS] != 0;
    if (resets) reset_runs(s, slot, resets == s.delivered * E_.J.n_ch);
    /* what this frame finds as rows 8..31 of its history: the frame behind it may need them at a reset */
    float *older_re = d_older_, *older_im = d_older_ + (size_t)NC * 24 * 64;
    HIP(hipMemcpy2DAsync(older_re, 24 * kRow, &d_estate_[0].qmf_re[8][0], kStatePitch, 24 * kRow, (size_t)NC, hipMemcpyDeviceToDevice, E_.stream));
    HIP(hipMemcpy2DAsync(older_im, 24 * kRow, &d_estate_[0].qmf_im[8][0], kStatePitch, 24 * kRow, (size_t)NC, hipMemcpyDeviceToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_header_, s.header, (size_t)NC * sizeof(xaac_sbr_header), hipMemcpyHostToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_frame_, s.frame, (size_t)NC * sizeof(xaac_sbr_frame), hipMemcpyHostToDevice, E_.stream));
    HIP(hipMemcpyAsync(d_eside_, s.eside, (size_t)NC * sizeof(xaac_esbr_side), hipMemcpyHostToDevice, E_.stream));
    if (mc_) { /* the in-place conversion of every element's channels in the frame's block, as the reference's layout has it */
      xaac_mc_core_in_batch cb = {N, E_.J.channel_config, d_out32_, d_qadj_, d_fcore_};
      XA(xaac_mc_core_from_out32_batch(E_.ctx, &cb));
    } else {
      xaac_esbr_core_in_batch cb = {NC, E_.J.n_ch, d_core_, d_fcore_};
      XA(xaac_esbr_core_from_pcm16_batch(E_.ctx, &cb));
    }
    xaac_esbr_sbr_batch b;
    memset(&b, 0, sizeof(b));
    b.n_ch = NC, b.core = d_fcore_, b.header = d_header_, b.frame = d_frame_, b.side = d_eside_, b.state = d_estate_, b.out = d_out_l_;
    b.status = E_.d_status[slot], b.workspace = d_ws_, b.workspace_bytes = ws_bytes_;
    tr_->attach(b, s);
    bool some_mono = false;
    xaac_esbr_pcm_out_batch ob = {N, 2048, d_out_l_, d_out_l_, E_.d_pcm[slot]}; /* a mono channel twice (api.c:3639-3660) */
    /* streams with and without PS in one step: the float PS launch copies left to right for those without (esbr_ps_kernel.hip) */
    if (with_ps) {
      HIP(hipMemcpyAsync(d_psf_, s.ps, (size_t)N * sizeof(xaac_ps_frame), hipMemcpyHostToDevice, E_.stream));
      b.ps_frame = d_psf_, b.ps_state = d_eps_, b.out_r = d_out_r_;
      ob.right = d_out_r_;
      some_mono = with_ps != s.delivered; /* streams without PS in this step: no right channel comes back for them (their right
                                             bank is left alone); their left samples are doubled on the host */
    } else if (!mono_) {
      ob.stride = 4096, ob.right = d_out_l_ + 2048;
    }
    XA(xaac_esbr_sbr_process_batch(E_.ctx, &b));
    if (mc_) { /* every element's planes into the frame's block, output channel order (ixheaacd_samples_sat_mc; no limiter: api.c:3381) */
      xaac_mc_pcm_out_batch mb;
      memset(&mb, 0, sizeof(mb));
      mb.n_streams = N, mb.n_ch = E_.J.n_ch, mb.stride = 2048, mb.planes = d_out_l_, mb.pcm = E_.d_pcm[slot];
      for (int c = 0; c < E_.J.n_ch; c++) mb.slot[c] = E_.J.slot[c];
      if (E_.J.map.kind == XAAC_OUT_MAP_DOWNMIX_STEREO) { /* -downmix:1: a sample's channels become its stereo pair on the way out */
        xaac_mc_pcm_out_map_batch xb;
        xb.out = mb, xb.map = E_.J.map;
        XA(xaac_mc_pcm16_from_float_map_batch(E_.ctx, &xb));
      } else {
        XA(xaac_mc_pcm16_from_float_batch(E_.ctx, &mb));
      }
    } else {
      XA(xaac_esbr_pcm16_from_float_batch(E_.ctx, &ob));
    }
    return {E_.d_pcm[slot], (size_t)N * E_.J.per * E_.J.out_ch * 2, false, some_mono, NC};
  }

 private:
  static constexpr size_t kRow = 64 * sizeof(float), kStatePitch = sizeof(xaac_esbr_state), kPlanePitch = 2048 * sizeof(float);

  /* rows between the channels' places and the scratch planes, `in` to the planes or back: a strided 2-D copy per move over
     every channel, or a copy per move for unit u's channel */
  void move_rows(const ResetSet &R, int u, bool in, std::initializer_list<RowMove> moves) {
    for (const RowMove &m : moves) {
      if (R.gathered) {
        float *plane = m.scratch + (size_t)u * 2048;
        void *home = static_cast<char *>(m.home) + (size_t)R.chs[(size_t)u] * m.pitch;
        HIP(hipMemcpyAsync(in ? (void *)plane : home, in ? home : (void *)plane, m.rows * kRow, hipMemcpyDeviceToDevice, E_.stream));
      } else if (in) {
        HIP(hipMemcpy2DAsync(m.scratch, kPlanePitch, m.home, m.pitch, m.rows * kRow, (size_t)E_.NC, hipMemcpyDeviceToDevice, E_.stream));
      } else {
        HIP(hipMemcpy2DAsync(m.home, m.pitch, m.scratch, kPlanePitch, m.rows * kRow, (size_t)E_.NC, hipMemcpyDeviceToDevice, E_.stream));
      }
    }
  }

  /* ixheaacd_sbr_dec_reset for Path A (sbrdecoder.c:175-236): the transposer's parameters from the new band tables (its
     two delay lines cleared, hbe_trans.c:102-222; with -esbr_hq:1 ixheaacd_dft_hbe_data_reinit), then its two runs over rows
     8..39 and 40..71 of the QMF buffer (the codec bank's num_time_slots is 32) as the frame before left it: rows 8..31 are
     what that frame found as its history rows 8..31 (d_older_), rows 32..71 are the state's history.  The second run's last
     eight output rows are the state's ph rows (bands outside the transposer's range keep what they held).
     `every`: all the step's delivered streams reset (every stream's first frame) -- the QMF transposer then runs on the states
     where they are and the rows move with strided copies over all channels.  Otherwise only some streams reset (their headers
     changed: independent streams do that at different frames), or the transposer has no strided form: the same sequence on
     those streams' channels gathered into a compact batch -- their transposer states into a second array, their rows into
     the first slots of the scratch planes, the two runs over that batch, states and ph rows back to their places.  The other
     streams' states are not touched. */
  void reset_runs(const Staging &s, int slot, bool every) {
    const int NC = E_.NC, n_ch = E_.J.n_ch;
    ResetSet R;
    R.gathered = tr_->always_gathers() || !every;
    if (R.gathered)
      for (int i = 0; i < NC; i++)
        if (s.status[(size_t)(i / n_ch)] == 0 && s.flags[E_.J.flag_row(i) * XAAC_SBR_FLAG_WORDS + XAAC_SBR_FLAG_RESET] != 0) R.chs.push_back(i);
    R.n = R.gathered ? (int)R.chs.size() : NC;
    if (!sc_.q_re) {
      sc_.q_re = E_.mem.dev<float>((size_t)NC * 2 * 2048), sc_.pv_re = E_.mem.dev<float>((size_t)NC * 2 * 2048);
      sc_.q_im = sc_.q_re + (size_t)NC * 2048, sc_.pv_im = sc_.pv_re + (size_t)NC * 2048;
      sc_.idx = E_.mem.dev<int32_t>((size_t)NC);
    }
    float *older_re = d_older_, *older_im = d_older_ + (size_t)NC * 24 * 64;
    xaac_esbr_state *st = d_estate_;
    tr_->new_parameters(s, R);
    HIP(hipStreamSynchronize(E_.stream));
    for (int u = 0; u < R.units(); u++) {
      tr_->stage(s, R, sc_, u);
      /* run 1: buffer rows 8..39 = the 24 older rows, then the state's first eight */
      move_rows(R, u, true, {{sc_.q_re, older_re, 24 * kRow, 24}, {sc_.q_im, older_im, 24 * kRow, 24},
                             {sc_.q_re + 24 * 64, &st[0].qmf_re[0][0], kStatePitch, 8}, {sc_.q_im + 24 * 64, &st[0].qmf_im[0][0], kStatePitch, 8}});
    }
    tr_->upload(R, sc_);
    tr_->run(R, sc_, E_.d_status[slot]);
    for (int u = 0; u < R.units(); u++) { /* run 2: buffer rows 40..71; its output rows 24..31 start from the state's ph rows */
      move_rows(R, u, true, {{sc_.q_re, &st[0].qmf_re[8][0], kStatePitch, 32}, {sc_.q_im, &st[0].qmf_im[8][0], kStatePitch, 32}});
      if (tr_->ph_rows_in())
        move_rows(R, u, true, {{sc_.pv_re + 24 * 64, &st[0].ph_re[0][0], kStatePitch, 8}, {sc_.pv_im + 24 * 64, &st[0].ph_im[0][0], kStatePitch, 8}});
    }
    tr_->run(R, sc_, E_.d_status[slot]);
    for (int u = 0; u < R.units(); u++) {
      move_rows(R, u, false, {{sc_.pv_re + 24 * 64, &st[0].ph_re[0][0], kStatePitch, 8}, {sc_.pv_im + 24 * 64, &st[0].ph_im[0][0], kStatePitch, 8}});
      tr_->back(R, u);
    }
  }

  const Env E_;
  const bool mono_, mc_; /* mc_: more than two channels, every channel element's channels through the batch as rows of their own */
  int16_t *d_core_ = nullptr;
  int32_t *d_out32_ = nullptr; /* mc_: the IMDCT's WORD32 rows and their qshift_adj, what the in-place conversion starts from */
  int8_t *d_qadj_ = nullptr;
  xaac_sbr_header *d_header_;
  xaac_sbr_frame *d_frame_;
  xaac_esbr_side *d_eside_;
  xaac_esbr_state *d_estate_;
  xaac_ps_frame *d_psf_ = nullptr;
  xaac_esbr_ps_state *d_eps_ = nullptr;
  float *d_fcore_, *d_out_l_, *d_out_r_ = nullptr;
  float *d_older_; /* [2][NC][24][64]: rows 8..31 of the QMF history as the frame before found them (see the reset) */
  ResetScratch sc_ = {nullptr, nullptr, nullptr, nullptr, nullptr}; /* made at the first reset */
  std::unique_ptr<Transposer> tr_;
  void *d_ws_;
  uint64_t ws_bytes_;
};

/* What every kind of stream shares in a shard: the context and the `stream` / `down` pair with their events, spectra, window
   info and overlap on the device, the two PCM / status slots, the narrowed copy of the spectra, the step's PCM taken one step
   late (Pending / consume), -profile, -verify and the counters.  The parse side feeds it, a tools stage may run in front, and
   the chain picked at construction does the rest: the step loop has no test of the kind of stream. */
class ShardDriver {
 public:
  ShardDriver(const Job &J, Shard &S, ShardOwner &mem) : J_(J), S_(S), N_(S.n), NC_(S.n * J.n_ch) {
    const int N = N_, NC = NC_;
    stream_ = mem.stream();
    ctx_ = mem.context(stream_);
    XA(xaac_warm_up(ctx_)); /* the kernels' code objects are on the device before the first batch (and the run's clock) */
    /* device-resident state and per-step device buffers */
    int32_t *d_overlap = mem.dev<int32_t>((size_t)NC * 512);
    d_spec_ = mem.dev<int32_t>((size_t)NC * 1024);
    xaac_ovl_state *d_ovl = mem.dev<xaac_ovl_state>((size_t)NC);
    d_ics_ = mem.dev<xaac_ics_info>((size_t)NC);
    /* PCM and status of a step in two sets: the copy down of step k (a second stream) runs beside the copies up and the kernels
       of step k + 1 */
    down_ = mem.stream();
    Env E = {J, N, NC, mem, ctx_, stream_, d_spec_, {nullptr, nullptr}, {nullptr, nullptr}, {}};
    for (int k = 0; k < 2; k++) {
      E.d_pcm[k] = mem.dev<int16_t>((size_t)N * J.per * J.out_ch), h_pcm_[k] = mem.pinned<int16_t>((size_t)N * J.per * (J.out_ch > 2 ? J.out_ch : 2));
      E.d_status[k] = mem.dev<int32_t>((size_t)NC), h_status_[k] = mem.pinned<int32_t>((size_t)NC);
      ev_kernels_[k] = mem.event(), ev_down_[k] = mem.event();
    }
    memset(&E.imdct, 0, sizeof(E.imdct));
    /* more than two channels: every channel a row of its own (ch_fac 1), the rows of a stream in output channel order --
       send_up puts them there --, so that the overlap, window state and qshift_adj rows and the planar block the limiter reads are
       in that order too */
    E.imdct.n_ch = NC, E.imdct.ch_fac = J.channel_config ? 1 : J.n_ch, E.imdct.spec = d_spec_, E.imdct.ics = d_ics_, E.imdct.overlap = d_overlap, E.imdct.state = d_ovl;
    for (int k = 0; k < 2; k++) d_status_[k] = E.d_status[k];
    if (J.gputools) tools_.reset(new ToolsStage(E));
    /* the chain, picked once */
    if (!J.sbr) chain_.reset(new LcChain(E));
    else if (J.esbr) chain_.reset(new EsbrChain(E));
    else chain_.reset(new SbrChain(E));
    parse_.reset(new ParseSide(J, S, mem, chain_->wants()));
    S.pcms.assign((size_t)(J.list_mode ? N : 1), std::vector<int16_t>()); /* every stream's output (-ilist), or stream 0's */
    ended_.assign((size_t)N, 0), refused_.assign((size_t)N, 0);
    if (J.channel_config)
      for (auto &h : h_ics_routed_) h = mem.pinned<uint8_t>((size_t)NC * 2);
  }

  void run() {
    constexpr int T = ParseSide::T;
    const auto t_all = std::chrono::steady_clock::now();
    t_first_ = t_all;
    bool first = true;
    parse_->start();
    for (int step = 0;; step++) {
      const int which = step % (3 * T), slot = step & 1;
      if (step % T == 0) parse_->wait(step / T);
      const Staging &s = parse_->step(which);
      if (s.delivered == 0) break;
      if (s.delivered != N_) note_ended(s);
      if (first && tools_) tools_->begin(parse_->parsers());
      if (step % T == 0) parse_->start(); /* the next group's frames are parsed while the GPU works on this one's */
      t_phase_ = std::chrono::steady_clock::now();
      if (J_.routed_up()) send_up_routed(s, which);
      else send_up(s);
      lap(0);
      if (tools_) tools_->run(slot);
      const StepOut o = chain_->run(s, slot);
      lap(1);
      bring_down(o, slot);
      consume(); /* the step before this one: its PCM has been on its way while this step's work was queued */
      pending_ = {true, first, slot, &s, o};
      if (J_.profile) consume(); /* phase timing wants one step at a time */
      first = false;
    }
    consume();
    parse_->stop();
    const auto t_end = std::chrono::steady_clock::now();
    S_.wall = std::chrono::duration<double>(t_end - t_all).count();
    S_.steady = std::chrono::duration<double>(t_end - t_first_).count();
    chain_->finish(S_.pcms);
  }

 private:
  void lap(int k) { /* -profile: copies up, kernels, copies down, host work on the PCM */
    if (!J_.profile) return;
    HIP(hipStreamSynchronize(stream_));
    const auto now = std::chrono::steady_clock::now();
    S_.phase_s[k] += std::chrono::duration<double>(now - t_phase_).count();
    t_phase_ = now;
  }
  void note_ended(const Staging &s) {
    if (!J_.list_mode) die("streams of different lengths in one batch");
    for (int i = 0; i < N_; i++)
      if (s.status[(size_t)i] != 0 && !ended_[(size_t)i]) { /* this stream is over: the other rows go on, its own run idle */
        ended_[(size_t)i] = 1;
        chain_->stream_ended(i);
      }
  }
  void send_up(const Staging &s) {
    { /* only the leading lines that are not zero in every delivered row go up, and what the device array still holds beyond
         them from the step before (the host rows are zero there) */
      const int width = s.lines > lines_held_ ? s.lines : lines_held_;
      lines_held_ = s.lines;
      if (width >= 1024) HIP(hipMemcpyAsync(d_spec_, s.spec, (size_t)NC_ * 4096, hipMemcpyHostToDevice, stream_));
      else if (width > 0) HIP(hipMemcpy2DAsync(d_spec_, 4096, s.spec, 4096, (size_t)width * 4, (size_t)NC_, hipMemcpyHostToDevice, stream_));
    }
    HIP(hipMemcpyAsync(d_ics_, s.ics, (size_t)NC_ * 2, hipMemcpyHostToDevice, stream_));
    if (tools_) tools_->send_up(s);
  }
  /* more than two channels: bitstream channel c of every stream to row J.slot[c] of the stream's rows -- one strided copy per
     channel for the spectra; the window info through a routed copy of the step's own (its staging set comes round again 3 T
     steps later, long behind the copy) */
  void send_up_routed(const Staging &s, int which) {
    const int n_ch = J_.n_ch, N = N_;
    const int width = s.lines > lines_held_ ? s.lines : lines_held_;
    lines_held_ = s.lines;
    uint8_t *ics = h_ics_routed_[which];
    for (int c = 0; c < n_ch; c++) {
      const int to = J_.slot[c];
      if (width > 0)
        HIP(hipMemcpy2DAsync(d_spec_ + (size_t)to * 1024, (size_t)n_ch * 4096, s.spec + (size_t)c * 1024, (size_t)n_ch * 4096, (size_t)width * 4,
                             (size_t)N, hipMemcpyHostToDevice, stream_));
      for (int i = 0; i < N; i++) {
        const size_t a = ((size_t)i * n_ch + to) * 2, b = ((size_t)i * n_ch + c) * 2;
        ics[a] = s.ics[b], ics[a + 1] = s.ics[b + 1];
      }
    }
    HIP(hipMemcpyAsync(d_ics_, ics, (size_t)NC_ * 2, hipMemcpyHostToDevice, stream_));
    if (tools_) tools_->send_up(s);
  }
  void bring_down(const StepOut &o, int slot) {
    HIP(hipEventRecord(ev_kernels_[slot], stream_));
    HIP(hipStreamWaitEvent(down_, ev_kernels_[slot], 0));
    HIP(hipMemcpyAsync(h_pcm_[slot], o.d_pcm, o.bytes, hipMemcpyDeviceToHost, down_));
    if (o.status_rows) HIP(hipMemcpyAsync(h_status_[slot], d_status_[slot], (size_t)o.status_rows * 4, hipMemcpyDeviceToHost, down_));
    if (tools_) tools_->bring_down(slot, down_);
    HIP(hipEventRecord(ev_down_[slot], down_));
  }
  /* a kernel refused a frame of stream i: one file of a list must not take the others' output along, that stream's output ends
     in front of this frame, the batch goes on (its rows keep running; nothing more of them is written) */
  void refuse(size_t i, int row, const char *who) {
    if (!J_.list_mode) die((std::string("the ") + who + " refused a frame").c_str(), row);
    fprintf(stderr, "xaacdec_amd: stream %d: the %s refused a frame: the stream ends here\n", J_.index[(size_t)S_.lo + i], who);
    refused_[i] = 1;
  }
  void consume() { /* what a step leaves for the host once its copy down has arrived */
    if (!pending_.valid) return;
    const int N = N_, per = J_.per, out_ch = J_.out_ch, n_ch = J_.n_ch;
    HIP(hipEventSynchronize(ev_down_[pending_.slot]));
    int16_t *h_pcm = h_pcm_[pending_.slot];
    const int32_t *h_status = h_status_[pending_.slot];
    const int32_t *alive = pending_.s->status; /* 0: the stream delivered a frame in that step */
    if (tools_) {
      const int32_t *h_tstatus = tools_->status(pending_.slot);
      for (int k = 0; k < J_.n_els; k++)
        for (int i = 0; i < N; i++)
          if (h_tstatus[(size_t)k * N + i] < 0 && alive[i] == 0 && !refused_[(size_t)i]) /* as for the SBR kernels' refusals below */
            refuse((size_t)i, i, "AAC tools kernel");
    }
    /* (rows of streams that are over re-run their last staging rows: what the kernels say about those is not looked at) */
    for (int i = 0; i < pending_.out.status_rows; i++) {
      const size_t si = (size_t)(i / n_ch);
      /* side info the kernels do not take (the boundary's own checks: a parser's output passes them, a damaged payload that
         still parses may not) */
      if (h_status[i] < 0 && alive[si] == 0 && !refused_[si])
        refuse(si, i, "SBR kernels");
    }
    if (pending_.out.mono_twice) /* mono duplicated to stereo (api.c:3639-3660), from the back so that it can be done in place */
      for (long k = (long)N * 2048 - 1; k >= 0; k--) h_pcm[2 * k] = h_pcm[2 * k + 1] = h_pcm[k];
    if (pending_.out.some_mono) { /* the same for the streams of a PS batch whose frame carried no PS: the bank pair wrote their left
                                     samples into the interleaved rows and left the right ones alone */
      const int32_t *fl = pending_.s->flags;
      for (int i = 0; i < N; i++)
        if (alive[i] == 0 && fl[(size_t)i * XAAC_SBR_FLAG_WORDS + XAAC_SBR_FLAG_PS] == 0)
          for (int k = 0; k < 2048; k++) h_pcm[(size_t)i * 4096 + 2 * k + 1] = h_pcm[(size_t)i * 4096 + 2 * k];
    }
    lap(2);
    const size_t skip = pending_.first ? chain_->first_frame_skip() : 0;
    std::vector<std::vector<int16_t>> &pcms = S_.pcms;
    if (!(pending_.first && chain_->drops_first_frame()))
      for (size_t i = 0; i < pcms.size(); i++)
        if (alive[i] == 0 && !refused_[i]) pcms[i].insert(pcms[i].end(), h_pcm + i * per * out_ch + skip, h_pcm + (i + 1) * per * out_ch);
    for (int i = 1; J_.verify && i < N; i++)
      S_.mismatched += memcmp(h_pcm, h_pcm + (size_t)i * per * out_ch, (size_t)per * out_ch * 2) != 0;
    S_.frames += pending_.s->delivered;
    if (pending_.first) t_first_ = std::chrono::steady_clock::now(); /* the first step also loads the kernels' code objects */
    pending_.valid = false;
    lap(3);
  }

  const Job &J_;
  Shard &S_;
  const int N_, NC_;
  xaac_ctx *ctx_;
  hipStream_t stream_, down_;
  hipEvent_t ev_kernels_[2], ev_down_[2];
  int32_t *d_spec_;
  xaac_ics_info *d_ics_;
  int16_t *h_pcm_[2];
  uint8_t *h_ics_routed_[3 * ParseSide::T] = {nullptr};
  int32_t *d_status_[2], *h_status_[2];
  std::unique_ptr<ToolsStage> tools_;
  std::unique_ptr<Chain> chain_;
  std::unique_ptr<ParseSide> parse_;
  int lines_held_ = 0; /* leading spectral lines that may be non-zero in d_spec */
  std::chrono::steady_clock::time_point t_phase_, t_first_;
  std::vector<char> ended_;
  std::vector<uint8_t> refused_; /* -ilist: streams a kernel refused a frame of (their output has ended) */
  struct Pending { /* what a step leaves for the host once its copy down has arrived */
    bool valid, first;
    int slot;
    const Staging *s;
    StepOut out;
  } pending_ = {false, false, 0, nullptr, {nullptr, 0, false, false, 0}};
};

/* a look at a stream's frame 0: sampling rate, channels, SBR or not (api.c:3369-3373: the SBR tools run for frames with an SBR
   payload; a stream at 24 kHz and below has an SBR decoder object by implicit signalling, api.c:2160, which is never called
   without payloads).  `report`: the parser's code goes into the message (the batch's first stream). */
struct FirstFrame {
  int rate, n_ch, sbr;
  int channel_config; /* 3 .. 6: several channel elements (the frame's sequence is the configuration's, or it would not have parsed); else 0 */
};
FirstFrame first_frame(const std::vector<uint8_t> &data, bool report) {
  xaac_adts_header hdr;
  if (xaac_adts_parse_header(data.data(), data.size(), &hdr)) die("ADTS header");
  xaac_parser *probe = nullptr;
  XA(xaac_parser_create(&probe));
  static thread_local xaac_core_frame cf[4];
  size_t used = 0;
  int32_t n_elems = 0;
  const int32_t rc = xaac_parse_adts_frame_mc(probe, data.data(), data.size(), 1, cf, 4, &n_elems, &used);
  if (rc) die("first frame", report ? rc : 0);
  xaac_parser_destroy(probe);
  int n_ch = 0, sbr = 0;
  for (int k = 0; k < n_elems; k++) n_ch += cf[k].n_ch, sbr |= cf[k].sbr_bytes > 0;
  return {hdr.sampling_rate, n_ch, sbr, n_elems > 1 ? hdr.channel_config : 0};
}

/* Where the reference puts the channels of channel_config 3 .. 6 and the mask it writes into the WAV header
   (ixheaacd_get_channel_mask, common_lpfuncs.c:107-173, through the slot / element routing of api.c:3176-3177): the first CPE
   takes the first two output channels, then the first SCE, the LFE, the second CPE, the second SCE.  slot[c]: output channel of
   bitstream channel c. */
uint32_t layout_of(int channel_config, int *slot) {
  static const int k_slot[4][6] = {{2, 0, 1}, {2, 0, 1, 3}, {2, 0, 1, 3, 4}, {2, 0, 1, 4, 5, 3}};
  static const uint32_t k_mask[4] = {0x7, 0x107, 0x37, 0x3f};
  for (int c = 0; c < 6; c++) slot[c] = k_slot[channel_config - 3][c];
  return k_mask[channel_config - 3];
}

void decode_shard(const Job &J, Shard &S) {
  S.first_frames = S.n;
  S.mem.reset(new ShardOwner(S.device)); /* main releases it behind the run's clock: the rates it prints never held a tear-down */
  ShardDriver(J, S, *S.mem).run();
}

/* the flags that decide what a kind of stream goes through */
struct Flags {
  int esbr, hq, gputools, mcsbr, downmix, dmix, tostereo, lim_off;
  int drc; /* any -drc_* flag was given */
  xaac_drc_config drc_cfg;
};

/* One group of a run: the streams of one kind -- an -ilist of mono and stereo streams has as many groups as kinds, in the order in
   which the list first names them; every other run has one -- with its Job, its shards over the devices and what its files' headers
   say.  Groups share nothing but the parser library's team of threads. */
struct Group {
  FirstFrame kind;
  Job J;
  std::vector<Shard> shards;
  uint32_t mask;
  int out_rate;
  long frames() const {
    long f = 0;
    for (const Shard &S : shards) f += S.frames;
    return f;
  }
};

/* What the flags mean for one kind of stream, as they mean it for a list of that kind alone: the part of the Job that follows
   from the kind.  -> nullptr, or why this decoder does not take the output stage flags on that kind (nothing has been opened or
   written yet; the caller says which file it was). */
const char *fill_job(Job &J, const FirstFrame &f0, const Flags &F) {
  const int n_ch = f0.n_ch, sbr = f0.sbr;
  if (f0.channel_config && sbr) {
    if (!F.mcsbr) die("multichannel SBR (an SBR payload in a stream of more than two channels) is not supported");
    if (F.hq) die("-mcsbr:1 with -esbr_hq:1 (the DFT transposer in a stream of more than two channels) is not supported");
    if (!F.esbr) die("-mcsbr:1 with -esbr:0 (the fixed-point SBR tools in a stream of more than two channels) is not supported");
    if (2 * f0.rate > 48000) die("-mcsbr:1 with a down-sampled bank (an output rate above 48 kHz) is not supported");
  }
  /* above a 24 kHz core the reference goes over to the down-sampled synthesis bank and writes at the core's rate
     (sbrdec_initfuncs.c:622); the chains of this decoder write at twice the core's rate, so such a stream is not taken */
  if (sbr && !f0.channel_config && 2 * f0.rate > 48000)
    return "SBR with a down-sampled bank (an output rate above 48 kHz) is not supported";
  const int downmix = F.downmix, dmix = F.dmix, tostereo = F.tostereo;
  if (downmix && dmix) return "-downmix:1 together with -dmix:1 is not supported";
  if (downmix && n_ch <= 2) return "-downmix:1 on a stream of one or two channels is not supported (there is nothing to mix down)";
  if (downmix && (n_ch > 6 || !f0.channel_config)) return "-downmix:1 takes channel configurations 3 .. 6";
  if (dmix && (sbr || n_ch > 2)) return "-dmix:1 on a stream with SBR or with more than two channels is not supported";
  if (dmix && tostereo && n_ch == 1) return "-dmix:1 together with -tostereo:1 on a mono stream is not supported";
  if (F.drc && sbr) return "a -drc_* flag on a stream with SBR (the QMF-domain branch of dynamic range control) is not supported";
  if (F.drc && (f0.channel_config || n_ch > 2)) return "a -drc_* flag on a stream of more than two channels is not supported";

  xaac_out_map map;
  memset(&map, 0, sizeof(map));
  if (downmix) { /* the frame's channel elements and their slots (layout_of): SCE CPE [SCE | CPE [LFE]] */
    static const int k_type[4][4] = {{0, 1}, {0, 1, 0}, {0, 1, 1}, {0, 1, 1, 3}}, k_slot[4][4] = {{2, 0}, {2, 0, 3}, {2, 0, 3}, {2, 0, 4, 3}};
    map.kind = XAAC_OUT_MAP_DOWNMIX_STEREO, map.matrix = n_ch == 6, map.n_elements = n_ch == 3 ? 2 : (n_ch == 6 ? 4 : 3);
    for (int k = 0; k < map.n_elements; k++) map.element_type[k] = k_type[n_ch - 3][k], map.element_slot[k] = k_slot[n_ch - 3][k];
  } else if (dmix && n_ch == 2) {
    map.kind = tostereo ? XAAC_OUT_MAP_MONO_MIX_DUP : XAAC_OUT_MAP_MONO_MIX;
  } else if (tostereo && n_ch == 1 && !sbr) {
    map.kind = XAAC_OUT_MAP_DUP_STEREO;
  } /* (everything else is a no-op in the reference too) */
  J.hq = F.hq, J.gputools = F.gputools;
  J.n_ch = n_ch, J.sbr = sbr, J.rate = f0.rate, J.per = sbr ? 2048 : 1024;
  J.esbr = sbr ? F.esbr : 0;       /* AAC-LC streams decode the same either way */
  J.lim_off = sbr ? 0 : F.lim_off; /* no limiter on the SBR paths: the flag changes nothing there */
  J.drc = F.drc, J.drc_cfg = F.drc_cfg;
  /* SBR streams come out in stereo (PS, or the mono column twice); AAC-LC, and everything with more than two channels, as coded;
     with a map, what the map leaves */
  J.out_ch = map.kind == XAAC_OUT_MAP_MONO_MIX ? 1 : (map.kind != XAAC_OUT_MAP_NONE ? 2 : (sbr && !f0.channel_config ? 2 : n_ch));
  J.map = map;
  J.channel_config = f0.channel_config;
  memset(J.slot, 0, sizeof(J.slot));
  J.n_els = 1, J.first_ch[0] = J.first_ch[1] = J.first_ch[2] = J.first_ch[3] = 0;
  if (J.channel_config) { /* SCE CPE [SCE | CPE [LFE]] */
    static const int k_first[4][4] = {{0, 1}, {0, 1, 3}, {0, 1, 3}, {0, 1, 3, 5}};
    J.n_els = J.channel_config == 3 ? 2 : (J.channel_config == 6 ? 4 : 3);
    for (int k = 0; k < 4; k++) J.first_ch[k] = k_first[J.channel_config - 3][k];
  }
  for (int c = 0; c < 8; c++) {
    J.el_of_ch[c] = 0;
    for (int k = 1; k < J.n_els; k++)
      if (c >= J.first_ch[k]) J.el_of_ch[c] = k;
  }
  return nullptr;
}

/* the size the parser library's team takes when nobody names one (host/xaac_parse.cpp: batch_threads, less its look at a cgroup's
   quota): what the groups of a mixed list share when -threads is not given -- one default for the run, not one per group */
int default_parser_threads() {
  const int hw = (int)std::thread::hardware_concurrency();
  int t = hw >= 4 ? (hw / 2 > 48 ? 48 : hw / 2) : (hw > 0 ? hw : 1);
  cpu_set_t set;
  const int usable = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 0;
  if (usable > 0 && t > 2 * usable) t = 2 * usable;
  return t;
}

const char *const k_map_name[] = {"none", "downmix", "mono", "mono_dup", "dup"};

void print_shards(const std::vector<Shard> &shards, int group) { /* -plan: a group's split; group >= 0: with the group's number */
  for (size_t r = 0; r < shards.size(); r++) {
    printf("%s{\"device\": %d, ", r ? ", " : "", shards[r].device);
    if (group >= 0) printf("\"group\": %d, ", group);
    printf("\"lo\": %d, \"n\": %d}", shards[r].lo, shards[r].n);
  }
}
/* -plan: what a group's streams come out as (the keys a run of one group has had all along) */
void print_plan_kind(const Group &G) {
  const Job &J = G.J;
  printf("\"channels\": %d, \"sbr\": %d, \"esbr\": %d, \"out_channels\": %d, \"out_map\": \"%s\", \"limiter\": %d, \"wav_header\": \"%s\"", J.n_ch,
         J.sbr, J.esbr, J.out_ch, k_map_name[J.map.kind], !J.sbr && !J.lim_off, J.out_ch > 2 ? "extensible68" : "pcm44");
  if (J.drc) printf(", \"drc\": {\"cut\": %d, \"boost\": %d, \"target_level\": %d}", J.drc_cfg.cut, J.drc_cfg.boost, J.drc_cfg.target_level);
}

}  // namespace

int main(int argc, char **argv) {
  std::string in, out, ilist, odir;
  int copies = 1, threads = 0, quiet = 0, verify = 0, profile = 0, esbr = 1, gpus = 1, device0 = 0, plan = 0, wrap = 0, hq = 0, gputools = 0, mcsbr = 0;
  int downmix = 0, dmix = 0, tostereo = 0, lim_off = 0, serialgroups = 0;
  bool bad_flag = false;
  int drc = 0;
  xaac_drc_config drc_cfg = {100, 100, 108}; /* what the reference keeps for the flags not given (api.c:477-481) */
  const struct {
    const char *name;
    int *value;
  } out_flags[] = {{"-downmix:", &downmix}, {"-dmix:", &dmix}, {"-tostereo:", &tostereo}, {"-peak_limiter_off:", &lim_off}};
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    bool taken = false;
    for (const auto &f : out_flags)
      if (a.rfind(f.name, 0) == 0) {
        const std::string v = a.substr(strlen(f.name));
        if (v != "0" && v != "1") reject((std::string(f.name) + "0 or " + f.name + "1").c_str());
        *f.value = v == "1", taken = true;
      }
    if (taken) continue;
    /* the reference's -drc_* flags (test/decoder/ixheaacd_main.c:507-538, api.c:629-673): each of them switches DRC on */
    if (a.rfind("-drc_cut_fac:", 0) == 0 || a.rfind("-drc_boost_fac:", 0) == 0) {
      const bool cut = a[5] == 'c';
      const float v = (float)atof(a.c_str() + (cut ? 13 : 15));
      if (!(v >= 0 && v <= 1)) reject(cut ? "-drc_cut_fac takes 0 .. 1" : "-drc_boost_fac takes 0 .. 1");
      (cut ? drc_cfg.cut : drc_cfg.boost) = (int32_t)(v * 100);
      drc = 1;
      continue;
    }
    if (a.rfind("-drc_target_level:", 0) == 0) {
      const long v = strtol(a.c_str() + 18, nullptr, 10);
      if (v < 0 || v > 127) reject("-drc_target_level takes 0 .. 127");
      drc_cfg.target_level = (int32_t)v, drc = 1;
      continue;
    }
    if (a.rfind("-drc_heavy_comp:", 0) == 0) {
      if (a != "-drc_heavy_comp:0") reject("-drc_heavy_comp:1 (heavy compression from DVB ancillary data) is not supported");
      drc = 1;
      continue;
    }
    if (a.rfind("-ifile:", 0) == 0) in = a.substr(7);
    else if (a.rfind("-ofile:", 0) == 0) out = a.substr(7);
    else if (a.rfind("-ilist:", 0) == 0) ilist = a.substr(7);
    else if (a.rfind("-odir:", 0) == 0) odir = a.substr(6);
    else if (a.rfind("-copies:", 0) == 0) copies = atoi(a.c_str() + 8);
    else if (a.rfind("-threads:", 0) == 0) threads = atoi(a.c_str() + 9);
    else if (a.rfind("-gpus:", 0) == 0) gpus = atoi(a.c_str() + 6);
    else if (a.rfind("-device:", 0) == 0) device0 = atoi(a.c_str() + 8);
    else if (a == "-plan") plan = 1;
    else if (a == "-wrap_devices") wrap = 1; /* shard r on device (k + r) mod the node's count: the -gpus host path on a box with fewer devices */
    else if (a == "-serialgroups:0") serialgroups = 0;
    else if (a == "-serialgroups:1") serialgroups = 1; /* the groups of a mixed list one after the other (to measure what side by side gains) */
    else if (a.rfind("-serialgroups", 0) == 0) bad_flag = true;
    else if (a == "-quiet") quiet = 1;
    else if (a == "-verify") verify = 1;
    else if (a == "-profile") profile = 1; /* synchronise behind every phase of a step and report the seconds spent in each */
    else if (a == "-gputools:0") gputools = 0;
    else if (a == "-gputools:1") gputools = 1;
    else if (a == "-mcsbr:0") mcsbr = 0;
    else if (a == "-mcsbr:1") mcsbr = 1;
    else if (a.rfind("-mcsbr", 0) == 0) die("-mcsbr:0 or -mcsbr:1");
    else if (a == "-esbr:0") esbr = 0;
    else if (a == "-esbr:1") esbr = 1;
    else if (a == "-esbr_hq:1") hq = 1;
    else if (a == "-esbr_hq:0") hq = 0;
    else if (a.rfind("-esbr", 0) == 0) die("-esbr:0 or -esbr:1 (and -esbr_hq:0 or -esbr_hq:1)");
  }
  std::vector<std::string> inputs;
  if (!ilist.empty()) {
    FILE *f = fopen(ilist.c_str(), "r");
    if (!f) die("fopen(-ilist)");
    char line[4096];
    while (fgets(line, sizeof(line), f)) {
      std::string sline(line);
      while (!sline.empty() && (sline.back() == '\n' || sline.back() == '\r' || sline.back() == ' ')) sline.pop_back();
      if (!sline.empty()) inputs.push_back(sline);
    }
    fclose(f);
    if (inputs.empty() || odir.empty()) die("-ilist needs paths and -odir");
    copies = 1, verify = 0;
  } else if (!in.empty()) {
    inputs.push_back(in);
  }
  if (bad_flag || inputs.empty() || (ilist.empty() && out.empty() && !plan) || copies < 1 || gpus < 1 || device0 < 0) {
    fprintf(stderr, "usage: xaacdec_amd -ifile:<in.aac> -ofile:<out.wav> [-esbr:0|1] [-esbr_hq:0|1] [-copies:N] [-threads:T] [-gpus:G] [-device:k] [-plan] [-gputools:0|1] [-mcsbr:0|1] [-quiet]\n"
                    "       xaacdec_amd -ilist:<file with one input path per line> -odir:<directory> [-serialgroups:0|1] [the flags above but -copies]\n"
                    "       [-downmix:0|1] [-dmix:0|1] [-tostereo:0|1] [-peak_limiter_off:0|1]\n"
                    "       [-drc_cut_fac:0..1] [-drc_boost_fac:0..1] [-drc_target_level:0..127]\n"
                    "  -ilist  mono and stereo streams of any sampling rate, with SBR or without, in one list: the streams of one kind are one group,\n"
                    "          the groups run side by side, every flag means for a group what it means for a list of that kind alone; a stream of\n"
                    "          more than two channels only beside streams of its own kind (refused before anything is written)\n"
                    "  -serialgroups:1  the groups of such a list one after the other on one thread (the same files)\n"
                    "  -mcsbr:1  decode HE-AAC streams of more than two channels (channel_config 3 .. 6, SBR per channel element; default flags only)\n"
                    "  -downmix:1  3 .. 6 channels come out in stereo (the reference's downmix matrix; a 44-byte stereo WAV header)\n"
                    "  -dmix:1  a stereo AAC-LC stream comes out mono, with -tostereo:1 the mono mix in both channels\n"
                    "  -tostereo:1  a mono AAC-LC stream comes out with its channel twice\n"
                    "  -peak_limiter_off:1  AAC-LC without the peak limiter (scale adjust + round16)\n"
                    "  -drc_cut_fac / -drc_boost_fac / -drc_target_level  MPEG-4 dynamic range control and level normalisation on AAC-LC mono\n"
                    "          and stereo streams (any of them switches it on; refused with SBR or more than two channels)\n");
    return 1;
  }
  std::vector<std::vector<uint8_t>> datas(inputs.size());
  for (size_t k = 0; k < inputs.size(); k++) {
    FILE *f = fopen(inputs[k].c_str(), "rb");
    if (!f) die("fopen(input)");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    datas[k].resize((size_t)n + 16);
    if (fread(datas[k].data(), 1, (size_t)n, f) != (size_t)n) die("fread");
    fclose(f);
    datas[k].resize((size_t)n);
  }
  /* the kinds of stream the run holds, in the order in which the list first names them, and which stream is of which */
  const bool list_mode = !ilist.empty();
  std::vector<Group> groups;
  std::vector<std::vector<int>> members;
  bool several_elements = false;
  for (size_t k = 0; k < datas.size(); k++) {
    const FirstFrame f = first_frame(datas[k], k == 0);
    several_elements = several_elements || f.channel_config != 0;
    size_t g = 0;
    for (; g < groups.size(); g++) {
      const FirstFrame &o = groups[g].kind;
      if (f.rate == o.rate && f.n_ch == o.n_ch && f.sbr == o.sbr && f.channel_config == o.channel_config) break;
    }
    if (g == groups.size()) {
      groups.emplace_back();
      groups.back().kind = f;
      members.emplace_back();
    }
    members[g].push_back((int)k);
  }
  /* a stream of several channel elements only beside streams of its own kind: its files have another header and its flags
     (-mcsbr, -downmix) refuse every other kind, so such a list is refused as a whole, here, before anything is opened or written */
  if (groups.size() > 1 && several_elements)
    die("-ilist: streams of different kinds (sampling rate, channels, channel configuration, SBR) in one batch");
  const bool mixed = groups.size() > 1;

  /* one Job per group.  The output stage flags are looked at per group: what this decoder does not take on one of them is refused
     here for the whole run, before a device is looked at or a file written (a mixed list: with the name of the first file it is
     refused for -- the groups stand in the order of their first files) */
  const Flags F = {esbr, hq, gputools, mcsbr, downmix, dmix, tostereo, lim_off, drc, drc_cfg};
  const int total = list_mode ? (int)datas.size() : copies;
  /* -threads:T is the whole run's: the groups of a mixed list take shares of it in proportion to their streams, one at least */
  const int team_threads = threads > 0 ? threads : default_parser_threads();
  int gpus_used = 0;
  for (size_t g = 0; g < groups.size(); g++) {
    Group &G = groups[g];
    Job &J = G.J;
    if (const char *why = fill_job(J, G.kind, F)) reject(mixed ? (inputs[(size_t)members[g][0]] + ": " + why).c_str() : why);
    const int N = list_mode ? (int)members[g].size() : copies;
    const int share = (int)((long)team_threads * N / total);
    J.threads = mixed ? (share > 1 ? share : 1) : threads;
    J.verify = verify, J.profile = profile, J.list_mode = list_mode;
    if (list_mode) {
      for (int k : members[g]) J.datas.push_back(std::move(datas[(size_t)k]));
      J.index = members[g];
    } else {
      J.datas = std::move(datas);
    }
    G.mask = J.channel_config ? layout_of(J.channel_config, J.slot) : 0;
    G.out_rate = J.sbr ? 2 * J.rate : J.rate;
    /* the split: contiguous stream ranges over the devices, as bench.py --gpus N splits over ranks (a shard without streams is
       not started: -gpus larger than a group uses as many devices as the group has streams) */
    const int g_gpus = gpus > N ? N : gpus;
    G.shards.resize((size_t)g_gpus);
    for (int r = 0; r < g_gpus; r++) {
      int lo, hi;
      shard_range(N, r, g_gpus, &lo, &hi);
      G.shards[(size_t)r].device = device0 + r, G.shards[(size_t)r].lo = lo, G.shards[(size_t)r].n = hi - lo;
    }
    gpus_used = g_gpus > gpus_used ? g_gpus : gpus_used;
  }
  gpus = gpus_used;
  const Group &G0 = groups[0]; /* the first listed stream's group: what the run's own lines say of the kind of stream */
  if (plan) { /* nothing below this line runs: no HIP call has been made */
    printf("{\"streams\": %d, \"gpus\": %d, ", total, gpus);
    print_plan_kind(G0);
    printf(", \"shards\": [");
    if (!mixed) print_shards(G0.shards, -1);
    for (size_t g = 0; mixed && g < groups.size(); g++) {
      if (g) printf(", ");
      print_shards(groups[g].shards, (int)g); /* (lo counts within the group) */
    }
    printf("]");
    if (mixed) { /* per group: what its files are, which list entries it holds and its own split */
      printf(", \"groups\": [");
      for (size_t g = 0; g < groups.size(); g++) {
        const Group &G = groups[g];
        printf("%s{\"rate\": %d, \"core_rate\": %d, \"streams\": %zu, \"threads\": %d, ", g ? ", " : "", G.out_rate, G.J.rate, members[g].size(), G.J.threads);
        print_plan_kind(G);
        printf(", \"list_index\": [");
        for (size_t k = 0; k < members[g].size(); k++) printf("%s%d", k ? ", " : "", members[g][k]);
        printf("], \"shards\": [");
        print_shards(G.shards, -1);
        printf("]}");
      }
      printf("], \"serialgroups\": %d", serialgroups);
    }
    printf("}\n");
    return 0;
  }
  {
    int have = 0;
    HIP(hipGetDeviceCount(&have));
    if (wrap && have > 0) {
      for (Group &G : groups)
        for (Shard &S : G.shards) S.device %= have;
    } else if (device0 + gpus > have) {
      fprintf(stderr, "xaacdec_amd: -device:%d -gpus:%d asks for devices %d..%d, the node has %d\n", device0, gpus, device0, device0 + gpus - 1, have);
      return 2;
    }
  }
  /* every (group, device) that has streams: one host thread with its own HIP stream and context.  -serialgroups:1: the groups one
     after the other (a group's shards side by side, as a run of that group alone has them) */
  const auto run_side_by_side = [](const std::vector<std::pair<const Job *, Shard *>> &work) {
    if (work.size() == 1) return decode_shard(*work[0].first, *work[0].second);
    std::vector<std::thread> team;
    for (const auto &w : work) team.emplace_back([w] { decode_shard(*w.first, *w.second); });
    for (auto &t : team) t.join();
  };
  const auto t_run = std::chrono::steady_clock::now();
  {
    std::vector<std::pair<const Job *, Shard *>> work;
    for (Group &G : groups) {
      for (Shard &S : G.shards) work.push_back({&G.J, &S});
      if (serialgroups) run_side_by_side(work), work.clear();
    }
    if (!work.empty()) run_side_by_side(work);
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_run).count();
  for (Group &G : groups)
    for (Shard &S : G.shards) S.mem.reset(); /* the shards are done: streams waited for, everything they allocated released */
  long frames = 0, mismatched = 0, first_frames = 0;
  double parse_s = 0, steady = 0;
  std::vector<std::vector<double>> phase_s(groups.size(), std::vector<double>(4, 0.0));
  for (size_t g = 0; g < groups.size(); g++)
    for (const Shard &S : groups[g].shards) {
      frames += S.frames, mismatched += S.mismatched, first_frames += S.first_frames;
      parse_s = S.parse_s > parse_s ? S.parse_s : parse_s;
      steady = S.steady > steady ? S.steady : steady;
      for (int k = 0; k < 4; k++) phase_s[g][(size_t)k] = S.phase_s[k] > phase_s[g][(size_t)k] ? S.phase_s[k] : phase_s[g][(size_t)k];
      /* -verify: every shard's copies were compared with its first one; the shards' first ones with the first shard's */
      if (verify && !list_mode && &S != &G0.shards[0]) mismatched += S.pcms[0] != G0.shards[0].pcms[0];
    }
  const std::vector<int16_t> &pcm = G0.shards[0].pcms[0];
  if (list_mode) { /* every stream with its own group's channel count, output rate and kind of header */
    for (const Group &G : groups)
      for (const Shard &S : G.shards)
        for (size_t i = 0; i < S.pcms.size(); i++) {
          std::string base = inputs[(size_t)G.J.index[(size_t)S.lo + i]];
          const size_t slash = base.find_last_of('/');
          if (slash != std::string::npos) base = base.substr(slash + 1);
          const size_t dot = base.find_last_of('.');
          if (dot != std::string::npos) base = base.substr(0, dot);
          write_wav(odir + "/" + base + ".wav", S.pcms[i], G.J.out_ch, G.out_rate, G.mask);
        }
  } else {
    write_wav(out, pcm, G0.J.out_ch, G0.out_rate, G0.mask);
  }
  if (!quiet && gpus > 1) { /* (the run's own line stays the last one); a device's rate: all it decoded over the longest of its shards */
    printf("{\"per_gpu_frames_per_s\": [");
    for (int r = 0; r < gpus; r++) {
      long f = 0;
      double w = 0;
      for (const Group &G : groups)
        if ((size_t)r < G.shards.size()) f += G.shards[(size_t)r].frames, w = G.shards[(size_t)r].wall > w ? G.shards[(size_t)r].wall : w;
      printf("%s%.1f", r ? ", " : "", w > 0 ? f / w : 0.0);
    }
    printf("]}\n");
  }
  if (!quiet) {
    /* a mixed list: frames and streams are the run's, the kind of stream is the first listed stream's group's, the groups follow */
    printf("{\"frames\": %ld, \"streams\": %d, \"wall_s\": %.4f, \"parse_s\": %.4f, \"frames_per_s\": %.1f, "
           "\"frames_per_s_after_first_step\": %.1f, \"mismatched_copies\": %ld, \"samples\": %zu, \"rate\": %d, \"sbr\": %d, "
           "\"channels\": %d, \"esbr\": %d, \"gpus\": %d",
           frames, total, wall, parse_s, frames / wall, frames > first_frames && steady > 0 ? (frames - first_frames) / steady : 0.0, mismatched,
           pcm.size() / G0.J.out_ch, G0.out_rate, G0.J.sbr, G0.J.n_ch, G0.J.esbr, gpus);
    for (size_t g = 0; mixed && g < groups.size(); g++) {
      const Group &G = groups[g];
      printf("%s{\"rate\": %d, \"channels\": %d, \"sbr\": %d, \"esbr\": %d, \"streams\": %zu, \"frames\": %ld}%s", g ? ", " : ", \"groups\": [", G.out_rate,
             G.J.n_ch, G.J.sbr, G.J.esbr, G.J.index.size(), G.frames(), g + 1 == groups.size() ? "]" : "");
    }
    printf("}\n");
  }
  for (size_t g = 0; profile && g < groups.size(); g++) { /* a mixed list: a line per group, with the group's number */
    printf("{");
    if (mixed) printf("\"group\": %zu, ", g);
    printf("\"h2d_s\": %.4f, \"kernels_s\": %.4f, \"d2h_s\": %.4f, \"host_pcm_s\": %.4f}\n", phase_s[g][0], phase_s[g][1], phase_s[g][2], phase_s[g][3]);
  }
  return mismatched ? 3 : 0;
}
