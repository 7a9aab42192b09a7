// alignasm_main.cpp -- `alignasm <input.paf>` command line, MI355X build.
//
// Keeps the reference's CLI surface and file contract (src/alignasm.cpp:30-75,487-490):
//   alignasm PAF_LOC [-t THREAD] [-a PAF_ALT_LOC] [-b ALT_BASELINE] [--non_skip_linkable]
//   -> <stem>.aln.paf, <stem>.aln.alt.paf, <stem>.aln.all.paf next to the input,
// and adds --max-paths K (MAX_PATH_COUNT, default 10000), --gpus N, --device D.
// -t sizes the host side (row-parallel PAF reader and writers; default: all hardware threads);
// the per-contig parallelism the reference drives with it now lives on the GPU.
//
// ---- The routes.  main() tries them in this order; each returns an Outcome: Written (the run is over, exit 0, or 3 with "writing
//      outputs failed"), GoOn (nothing was written, the next route that applies takes over) or Fatal (exit 1 / 2 / 3).  NOMEM, PARSE,
//      IO, INVAL are the library's AASM_E_* codes.  "exit 1" prints the library's text, as the reference does for a bad file;
//      "exit 2" prints "alignasm: solver failed (<rc>): <text>"; "exit 3" prints "alignasm: writing outputs failed: <text>".
//
//   1 no container   --device-reader --device-writer, --gpus <= 1, and no --alt (an empty alt file is none) or --device-alt
//        aasm_paf_read_device_rows            PARSE, IO, NOMEM -> GoOn;  other -> exit 2.
//        --device-alt with --alt: aasm_paf_merge_alt_device on the mapped alt file, the merged batch takes the resident one's place
//                                             PARSE (a text the device declines, or a bad one), IO, NOMEM -> GoOn;  other -> exit 2
//        Then the two stdout lines, once per run; after a device merge they wait until the route is sure to write, because the
//        plain command says nothing before its message for a bad --alt file, and a tag the solve rejects is such a file.
//        the warm-up threads are joined, then the device rows (below) without a container
//        GoOn from here on means the plain command: host reader, both flags off, its messages and exit codes.
//   - container read  aasm_paf_read_device with --device-reader (leaves the batch resident beside the container), else the host reader
//        with --device-reader a failure other than PARSE, IO -> exit 2;  every other failure -> exit 1
//        --alt or --gpus > 1 drop the resident batch;  a failed --alt merge -> exit 1
//   2 device writer  --device-writer
//        a batch that is not resident is uploaded in its cs form (a failed upload counts as NOMEM), then the row columns
//        NOMEM, PARSE -> GoOn;  other -> exit 2.  Then the device rows with the container.
//   3 resident       a resident batch is still held: aasm_solve_device, aasm_result_fetch, aasm_paf_write_outputs
//        NOMEM, PARSE -> GoOn;  other -> exit 2;  a failed write -> Written, exit 3
//   4 ranges         --gpus <= 1, contigs >= 64, records >= 65 536: a solver thread over contig ranges, the writer behind it
//        writer open fails -> exit 3;  PARSE from a range -> exit 1;  other solver failures -> exit 2;  a failed write -> Written, exit 3
//   5 one piece      everything else (--gpus > 1 too): aasm_solve_batch_multi, aasm_paf_write_outputs
//        PARSE -> exit 1;  other -> exit 2;  a failed write -> Written, exit 3
//
//   device rows (routes 1, 2): aasm_solve_device -> sizes -> export buffers -> export -> cut plans -> writer session
//        before the writer     NOMEM, PARSE -> GoOn;  other -> exit 2
//        aasm_writer_open      fails -> exit 3
//        aasm_writer_append_device    NOMEM -> GoOn;  without a container PARSE, INVAL -> GoOn too (a row that cannot be formatted:
//                                     that session checks every row before it writes one);  every other result -> Written
//
// ---- --timing prints one line to stderr after a Written outcome: records, contigs, then
//        read_s    start -> the batch is read (routes 2 - 5: merged and indexed too;  1 with --device-alt: merged on the device too)
//        solve_s   routes 1 - 3, 5: read -> results ready for the writer;  4: the solver thread's busy time
//        upload / device / fetch    1: wait for the arena / solve / sizes, export, plans;  2: the uploads / solve / sizes, export, plans;
//                  3: 0 / solve / fetch;  4: sums of the ranges' stats.reserved_f[0], [2], [1];  5: the same of the one solve
//        write_s   the time in the writers (4: summed over the ranges);  overlap_s  solve_s + write_s - (end - read)
//        total_s   start -> end;  container  0 when route 1 wrote the files, else 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <filesystem>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <algorithm>
#include <thread>
#include <vector>
#include <iostream>
#include <string>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>

#include "../../include/alignasm_amd.h"

using clk = std::chrono::steady_clock;
static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

static void usage(std::ostream &os) {
    os << "Usage: alignasm [--help] [--version] [--thread THREAD] [--alt PAF_ALT_LOC] [--alt_baseline ALT_BASELINE] "
          "[--non_skip_linkable] [--max-paths K] [--gpus N] [--device D] [--timing] [--host-ranges] [--device-reader] [--device-writer] [--device-alt] PAF_LOC\n\n"
          "Positional arguments:\n  PAF_LOC              Location of PAF file [required]\n\n"
          "Optional arguments:\n  -h, --help           shows help message and exits\n  -v, --version        prints version information and exits\n"
          "  -t, --thread THREAD  Number of host threads for reading / writing PAF [default: all]\n"
          "  -a, --alt PAF_ALT_LOC  Location of alternative PAF file\n"
          "  -b, --alt_baseline ALT_BASELINE  Baseline for coverage of alternative PAF file [default: 0.5]\n"
          "  --non_skip_linkable  no edge a -> b when a -> c -> b exists\n"
          "  --max-paths K        paths enumerated per contig (reference constant MAX_PATH_COUNT) [default: 10000]\n"
          "  --gpus N             shard contigs over N GPUs of this node [default: 1]\n"
          "  --device D           first HIP device ordinal [default: 0]\n"
          "  --timing             print read / solve / write wall time to stderr\n"
          "  --host-ranges        build the cs match ranges in the reader instead of on the GPU\n"
          "  --device-reader      frame and parse the PAF rows on the GPU (not with --host-ranges)\n"
          "  --device-writer      format the output rows on the GPU (not with --host-ranges, not with --gpus above 1)\n"
          "  --device-alt         with --device-reader --device-writer: merge the --alt file on the GPU into the resident batch\n"
          "                       (not with --host-ranges, not with --gpus above 1)\n";
}

struct Cli {
    std::string paf_loc, alt_loc;
    aasm_opts opts;
    int gpus = 1;
    double alt_baseline = 0.5;
    bool use_alt = false;                                                       // --alt with a file that is not empty
    bool timing = false, host_ranges = false, device_reader = false, device_writer = false, device_alt = false;
};

// -1: go on with cli;  else the exit code (--help, --version, a usage error)
static int parse_args(int argc, char **argv, Cli &cli) {
    std::memset(&cli.opts, 0, sizeof cli.opts);
    cli.opts.max_paths = 10000;
    bool bad = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](const char *what) -> const char * {
            if (i + 1 >= argc) { std::cerr << what << ": missing value\n"; bad = true; return "0"; }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") { usage(std::cout); return 0; }
        else if (a == "-v" || a == "--version") { std::cout << "0.1.0\n"; return 0; }
        else if (a == "-t" || a == "--thread") aasm_set_host_threads(std::atoi(need("--thread")));
        else if (a == "--timing") cli.timing = true;
        else if (a == "--host-ranges") cli.host_ranges = true;
        else if (a == "--device-reader") cli.device_reader = true;
        else if (a == "--device-writer") cli.device_writer = true;
        else if (a == "--device-alt") cli.device_alt = true;
        else if (a == "-a" || a == "--alt") cli.alt_loc = need("--alt");
        else if (a == "-b" || a == "--alt_baseline") cli.alt_baseline = std::atof(need("--alt_baseline"));
        else if (a == "--non_skip_linkable") cli.opts.non_skip_linkable = 1;
        else if (a == "--max-paths") cli.opts.max_paths = std::atoi(need("--max-paths"));
        else if (a == "--gpus") cli.gpus = std::atoi(need("--gpus"));
        else if (a == "--device") cli.opts.device = std::atoi(need("--device"));
        else if (!a.empty() && a[0] == '-') { std::cerr << "Unknown argument: " << a << "\n"; bad = true; }
        else if (cli.paf_loc.empty()) cli.paf_loc = a;
        else { std::cerr << "Maximum number of positional arguments exceeded\n"; bad = true; }
    }
    if (cli.host_ranges && cli.device_reader) { std::cerr << "--device-reader: not with --host-ranges\n"; bad = true; }
    if (cli.host_ranges && cli.device_writer) { std::cerr << "--device-writer: not with --host-ranges\n"; bad = true; }
    if (cli.host_ranges && cli.device_alt) { std::cerr << "--device-alt: not with --host-ranges\n"; bad = true; }
    if (cli.gpus > 1 && cli.device_writer) { std::cerr << "--device-writer: not with --gpus above 1\n"; bad = true; }
    if (cli.gpus > 1 && cli.device_alt) { std::cerr << "--device-alt: not with --gpus above 1\n"; bad = true; }
    if (bad || cli.paf_loc.empty()) { usage(std::cerr); return 1; }             // alignasm.cpp:59-65
    for (const std::string *loc : {&cli.paf_loc, &cli.alt_loc}) {               // :67-72, :186-201
        if (loc->empty() || std::filesystem::path(*loc).extension() == ".paf") continue;
        std::cerr << "Wrong PAF file : " << std::filesystem::absolute(*loc);
        usage(std::cerr);
        return 1;
    }
    if (!cli.alt_loc.empty()) {
        std::error_code ec;
        auto sz = std::filesystem::file_size(cli.alt_loc, ec);
        cli.use_alt = !(!ec && sz == 0);                                        // empty file == no --alt
    }
    return -1;
}

struct Timing {
    clk::time_point t0, t1, t2;                                                 // start, batch read, results ready for the writer
    double upload_s = 0, device_s = 0, fetch_s = 0, solve_busy_s = 0, write_busy_s = 0;
    int container = 1;
    int64_t n_records = 0, n_contigs = 0;
};

static void print_timing(const Timing &t) {
    const auto t3 = clk::now();
    std::cerr << "alignasm timing: records " << t.n_records << " contigs " << t.n_contigs << " read_s " << secs(t.t0, t.t1) << " solve_s " << t.solve_busy_s
              << " (upload " << t.upload_s << " device " << t.device_s << " fetch " << t.fetch_s << ") write_s " << t.write_busy_s
              << " overlap_s " << (t.solve_busy_s + t.write_busy_s - secs(t.t1, t3)) << " total_s " << secs(t.t0, t3) << " container " << t.container << "\n";
}

struct Outcome {
    enum Kind { Written, GoOn, Fatal } kind;
    int rc;                                                                     // Written: the final AASM_* code;  Fatal: the exit code
};
// The three messages of a failed run.  write_failed is also said for a write that began and failed: that outcome is Written with the
// failing code, which ends in exit 3 as well, behind the --timing line.
static Outcome bad_input(const std::string &text) { std::cerr << text << "\n"; return {Outcome::Fatal, 1}; }   // e.g. "Missing cs:Z tag ..." (:165-168)
static Outcome solver_failed(int rc, const std::string &text) { std::cerr << "alignasm: solver failed (" << rc << "): " << text << "\n"; return {Outcome::Fatal, 2}; }
static Outcome write_failed(const std::string &text) { std::cerr << "alignasm: writing outputs failed: " << text << "\n"; return {Outcome::Fatal, 3}; }
// a failure on the device before anything is written: out of device memory, or a tag the device rejects (a bad file is no hot path),
// leave the next route to run from the container, with its messages and exit codes
static Outcome before_writer(int rc) { return rc == AASM_E_NOMEM || rc == AASM_E_PARSE ? Outcome{Outcome::GoOn, rc} : solver_failed(rc, aasm_last_error()); }
static void report_internal(int64_t n) { if (n) std::cerr << "alignasm: " << n << " contig(s) hit an internal error state\n"; }

// What a run holds.  A Fatal outcome leaves through the destructor; the successful end does not (main).
struct Run {
    const Cli &cli;
    Timing tm;
    std::vector<std::thread> warm;
    aasm_paf *paf = nullptr;                                                    // the container
    aasm_upload *up = nullptr;                                                  // the resident batch, seen through dev_view
    aasm_batch_in dev_view, view;
    std::string in, f_main, f_alt, f_all;
    bool said_read = false;
    int64_t held_contigs = -1;

    explicit Run(const Cli &c) : cli(c) {
        tm.t0 = tm.t1 = tm.t2 = clk::now();
        std::memset(&view, 0, sizeof view);
        const auto ap = std::filesystem::absolute(cli.paf_loc);
        auto with = [&](const char *ext) { return std::filesystem::path(ap).replace_extension(ext).string(); };
        in = ap.string(); f_main = with(".aln.paf"); f_alt = with(".aln.alt.paf"); f_all = with(".aln.all.paf");
    }
    ~Run() { join_warm(); drop_upload(); aasm_paf_free(paf); }
    // While the reader works: HIP start-up + the workspace arena of every GPU (sized from the file: ~3.7 bytes of arena
    // per byte of PAF text on whole-genome input; too small just means the solve allocates the rest itself).
    void warm_up() {
        std::error_code ec;
        double text = (double)std::filesystem::file_size(cli.paf_loc, ec);
        if (ec) text = 0;
        if (cli.use_alt) { const auto s2 = std::filesystem::file_size(cli.alt_loc, ec); if (!ec) text += (double)s2; }
        const int n = cli.gpus > 0 ? cli.gpus : 1, device = cli.opts.device;
        const int64_t per_gpu = (int64_t)(text * 3.7 / n) + ((int64_t)256 << 20);
        for (int g = 0; g < n; g++) warm.emplace_back([=] { (void)aasm_reserve_workspace(device + g, per_gpu); });
    }
    void join_warm() { for (auto &t : warm) if (t.joinable()) t.join(); }
    void drop_upload() { aasm_upload_free(up); up = nullptr; }
    // hold: the lines wait until the route is sure to write (said_held): the plain command says nothing before a bad --alt file's
    // message, and a tag the device merge leaves to the solve is such a file
    void say_read(int64_t n_contigs, int64_t n_records, bool hold = false) {    // once per run: a route that falls back has said it
        held_contigs = hold ? n_contigs : -1;
        if (!hold) say_lines(n_contigs);
        tm.n_contigs = n_contigs; tm.n_records = n_records;
        tm.t1 = tm.t2 = clk::now();
    }
    void say_held() { if (held_contigs >= 0) say_lines(held_contigs); held_contigs = -1; }
    void say_lines(int64_t n_contigs) {
        if (!said_read) std::cout << "File read complete" << std::endl << "Analyze PAF " << n_contigs << " data in parallel" << std::endl;   // :340, :349
        said_read = true;
    }
};

// The export buffers and cut plans of one result, on the device.
struct DevBufs {
    aasm_dev_out out;
    aasm_dev_cuts cuts;
    std::vector<void *> mem;
    bool oom = false;
    DevBufs() { std::memset(&out, 0, sizeof out); std::memset(&cuts, 0, sizeof cuts); }
    DevBufs(const DevBufs &) = delete;
    ~DevBufs() { for (void *q : mem) (void)hipFree(q); }
    template <class T> T *get(int64_t n) {
        void *q = nullptr;
        if (oom || hipMalloc(&q, (size_t)(n > 0 ? n * (int64_t)sizeof(T) : 8)) != hipSuccess) { (void)hipGetLastError(); oom = true; return nullptr; }
        mem.push_back(q);
        return (T *)q;
    }
    int alloc(const aasm_out_sizes &sz, int device) {
        (void)hipSetDevice(device);
        const int64_t C = sz.n_contigs;
        out.main_off = get<int64_t>(C + 1); out.alt_off = get<int64_t>(C + 1); out.all_path_off = get<int64_t>(C + 1);
        out.all_elem_off = get<int64_t>(sz.n_all_paths + 1); out.ctg_status = get<int32_t>(C);
        out.main_elems = get<aasm_out_elem>(sz.n_main); out.alt_elems = get<aasm_out_elem>(sz.n_alt); out.all_elems = get<aasm_out_elem>(sz.n_all_elems);
        cuts.main = get<aasm_cut_plan>(sz.n_main); cuts.alt = get<aasm_cut_plan>(sz.n_alt); cuts.all = get<aasm_cut_plan>(sz.n_all_elems);
        return oom ? AASM_E_NOMEM : AASM_OK;
    }
};

// The resident batch (run.up, run.dev_view) is solved in one piece and its rows are formatted on the device from the row columns:
// export -> cut plans -> device writer.  container: the host reader's, or nullptr (route 1).  The caller frees the batch.
static Outcome device_rows(Run &run, const aasm_row_cols &cols, const aasm_paf *container) {
    Timing &tm = run.tm;
    const int device = run.cli.opts.device;
    DevBufs bufs;
    aasm_result *res = nullptr;
    const auto tu = clk::now();
    int rc = aasm_solve_device(&run.dev_view, &run.cli.opts, nullptr, &res);
    const std::unique_ptr<aasm_result, decltype(&aasm_result_free)> free_res(res, aasm_result_free);
    const auto ts = clk::now();
    aasm_out_sizes sz;
    if (rc == AASM_OK) rc = aasm_result_sizes(res, &sz);
    if (rc == AASM_OK) rc = bufs.alloc(sz, device);
    if (rc == AASM_OK) rc = aasm_result_export(res, &sz, &bufs.out, nullptr);
    if (rc == AASM_OK) rc = aasm_cut_plans_device(&run.dev_view, &sz, &bufs.out, &bufs.cuts, device, nullptr);
    aasm_stats st;
    std::memset(&st, 0, sizeof st);
    if (rc == AASM_OK) (void)aasm_result_stats(res, &st);
    if (rc != AASM_OK) return before_writer(rc);
    (void)hipDeviceSynchronize();
    tm.t2 = clk::now();
    aasm_writer *wr = nullptr;
    rc = aasm_writer_open(run.f_main.c_str(), run.f_alt.c_str(), run.f_all.c_str(), &wr);
    if (rc != AASM_OK) return write_failed(aasm_last_error());
    rc = aasm_writer_append_device(wr, container, &run.dev_view, &cols, &sz, &bufs.out, &bufs.cuts, 0, 0, device);
    // Nothing was written and the session is as it was: out of memory; without a container also a row that cannot be formatted
    // (that session checks every row before it writes one).  With a container every other result is final.
    if (rc == AASM_E_NOMEM || (!container && (rc == AASM_E_PARSE || rc == AASM_E_INVAL))) { (void)aasm_writer_close(wr, 0); return {Outcome::GoOn, rc}; }
    tm.upload_s = secs(tm.t1, tu); tm.device_s = secs(tu, ts); tm.fetch_s = secs(ts, tm.t2); tm.solve_busy_s = secs(tm.t1, tm.t2);   // (upload: what the caller did since t1; fetch: sizes, export and plans)
    report_internal(st.n_internal_errors);
    run.say_held();
    std::cout << "Write output PAF file" << std::endl;                          // :487
    const std::string msg = rc != AASM_OK ? aasm_last_error() : "";
    const int crc = aasm_writer_close(wr, rc == AASM_OK ? 1 : 0);
    if (rc != AASM_OK) write_failed(msg);
    else if ((rc = crc) != AASM_OK) write_failed(aasm_last_error());
    tm.write_busy_s = secs(tm.t2, clk::now());
    tm.container = container ? 1 : 0;
    return {Outcome::Written, rc};
}

// --device-alt: the alt file, mapped, joins the resident batch on the device; the merged batch and its columns take their place
static int merge_alt_on_device(Run &run, aasm_row_cols &cols) {
    const std::string path = std::filesystem::absolute(run.cli.alt_loc).string();
    const int fd = ::open(path.c_str(), O_RDONLY);
    struct stat st;
    if (fd < 0 || ::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) { if (fd >= 0) ::close(fd); return AASM_E_IO; }
    void *m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) return AASM_E_IO;
    aasm_upload *merged = nullptr;
    aasm_batch_in merged_view;
    aasm_row_cols merged_cols;
    const int rc = aasm_paf_merge_alt_device(&run.dev_view, &cols, (const char *)m, (int64_t)st.st_size, run.cli.alt_baseline, 0, run.cli.opts.device, &merged, &merged_view, &merged_cols);
    ::munmap(m, (size_t)st.st_size);
    if (rc != AASM_OK) return rc;
    run.drop_upload();
    run.up = merged; run.dev_view = merged_view; cols = merged_cols;
    return AASM_OK;
}

// ---- 1: no container: read -> [--alt merge] -> solve -> sizes -> export -> cut plans -> device writer, all from resident arrays
static Outcome route_no_container(Run &run) {
    aasm_row_cols cols;
    int rc = aasm_paf_read_device_rows(run.in.c_str(), 0, run.cli.opts.device, nullptr, &run.up, &run.dev_view, &cols);
    if (rc == AASM_OK && run.cli.use_alt) rc = merge_alt_on_device(run, cols);
    if (rc == AASM_E_PARSE || rc == AASM_E_IO || rc == AASM_E_NOMEM) { run.drop_upload(); return {Outcome::GoOn, rc}; }
    if (rc != AASM_OK) return solver_failed(rc, aasm_last_error());
    run.say_read(run.dev_view.n_contigs, run.dev_view.n_records, run.cli.use_alt);
    // The device read holds the context's lock from start to end, so a warm-up that came second is still waiting to make the
    // arena.  It is waited for here: a solve that got the lock first would grow the arena block by block between its kernels.
    run.join_warm();
    const Outcome o = device_rows(run, cols, nullptr);
    run.drop_upload();
    return o;
}

// The container: the reader only indexes the rows; the cs tags are turned into match ranges on the GPU.
// device_reader: the rows are framed and parsed on the GPU, which leaves the batch resident (up, dev_view) beside the container.
static Outcome read_container(Run &run, bool device_reader) {
    const Cli &cli = run.cli;
    int rc = device_reader ? aasm_paf_read_device(run.in.c_str(), 0, cli.opts.device, &run.paf, &run.up, &run.dev_view)
                           : aasm_paf_read_opts(run.in.c_str(), cli.host_ranges ? 0 : AASM_READ_DEVICE_RANGES, &run.paf);
    if (rc != AASM_OK && device_reader && rc != AASM_E_PARSE && rc != AASM_E_IO) return solver_failed(rc, aasm_last_error());
    if (rc != AASM_OK) return bad_input(aasm_last_error());
    if (cli.use_alt || cli.gpus > 1) run.drop_upload();                         // the merge changes the records, shards are uploaded per GPU: on from the container
    if (cli.use_alt && aasm_paf_merge_alt(run.paf, std::filesystem::absolute(cli.alt_loc).c_str(), cli.alt_baseline) != AASM_OK) return bad_input(aasm_last_error());
    aasm_paf_batch(run.paf, &run.view);
    run.say_read(run.view.n_contigs, run.view.n_records);                       // (the warm-up threads are not waited for: the upload runs beside them, the solve takes the context's lock after them)
    return {Outcome::GoOn, AASM_OK};
}

// ---- 2: the batch - resident from --device-reader, else uploaded in its cs form from the container (after --alt: the merged one) -
//      and the container's row columns go through device_rows.
static Outcome route_device_writer(Run &run) {
    if (!run.up) {
        aasm_batch_in cs_view = run.view;
        cs_view.rng_qry_l = cs_view.rng_qry_r = cs_view.rng_ref_l = nullptr;
        if (aasm_upload_batch(&cs_view, run.cli.opts.device, &run.up, &run.dev_view) != AASM_OK) run.up = nullptr;
    }
    aasm_upload *up_rows = nullptr;
    aasm_row_cols cols;
    const int rc = run.up ? aasm_paf_upload_rows(run.paf, 0, run.view.n_contigs, run.cli.opts.device, &up_rows, &cols) : AASM_E_NOMEM;
    const Outcome o = rc == AASM_OK ? device_rows(run, cols, run.paf) : before_writer(rc);
    aasm_upload_free(up_rows);
    run.drop_upload();
    return o;
}

// the tail of routes 3 and 5: the whole result through the host writers
static Outcome write_outputs(Run &run, const aasm_batch_out &out) {
    report_internal(out.stats.n_internal_errors);
    std::cout << "Write output PAF file" << std::endl;                          // :487
    const int rc = aasm_paf_write_outputs(run.paf, &out, run.f_main.c_str(), run.f_alt.c_str(), run.f_all.c_str());
    if (rc != AASM_OK) write_failed(aasm_last_error());
    run.tm.write_busy_s = secs(run.tm.t2, clk::now());
    return {Outcome::Written, rc};
}

// ---- 3: the resident batch is solved in place and fetched
static Outcome route_resident(Run &run) {
    Timing &tm = run.tm;
    aasm_result *res = nullptr;
    aasm_batch_out out;
    std::memset(&out, 0, sizeof out);
    int rc = aasm_solve_device(&run.dev_view, &run.cli.opts, nullptr, &res);
    const auto ts = clk::now();
    if (rc == AASM_OK) rc = aasm_result_fetch(res, &out);
    aasm_result_free(res);
    run.drop_upload();
    if (rc != AASM_OK) return before_writer(rc);
    tm.t2 = clk::now();
    tm.device_s = secs(tm.t1, ts); tm.fetch_s = secs(ts, tm.t2); tm.solve_busy_s = secs(tm.t1, tm.t2);
    return write_outputs(run, out);
}

// ---- 4: one GPU: the file goes through in contig ranges of about equal record counts; while the GPU solves range k
//      (upload -> K0 .. K9 -> fetch) the host threads format and write the rows of range k - 1.  The three outputs
//      are appended to in contig order (aasm_writer_*), so the bytes are those of the one-piece path.
static bool ranges_apply(const Run &run) { return run.cli.gpus <= 1 && run.view.n_contigs >= 64 && run.view.n_records >= (1 << 16); }

static std::vector<int64_t> range_cuts(const aasm_batch_in &view) {
    const int n_chunks = (int)std::min<int64_t>(8, std::max<int64_t>(2, view.n_records / (1 << 19)));
    std::vector<int64_t> cut(n_chunks + 1, view.n_contigs);
    cut[0] = 0;
    for (int k = 1; k < n_chunks; k++) {
        const int64_t want = view.n_records * k / n_chunks;
        int64_t c = std::lower_bound(view.ctg_rec_off, view.ctg_rec_off + view.n_contigs + 1, want) - view.ctg_rec_off;
        cut[k] = std::min<int64_t>(std::max<int64_t>(c, cut[k - 1] + 1), view.n_contigs - (n_chunks - k));
    }
    return cut;
}

static Outcome route_ranges(Run &run) {
    Timing &tm = run.tm;
    const std::vector<int64_t> cut = range_cuts(run.view);
    const int n_chunks = (int)cut.size() - 1;
    aasm_writer *wr = nullptr;
    if (aasm_writer_open(run.f_main.c_str(), run.f_alt.c_str(), run.f_all.c_str(), &wr) != AASM_OK) return write_failed(aasm_last_error());
    std::vector<aasm_batch_out> outs(n_chunks);
    std::vector<int> rcs(n_chunks, AASM_OK);
    std::vector<std::string> errs(n_chunks);
    std::mutex mu;
    std::condition_variable cv;
    int solved = 0;                                                             // ranges [0, solved) are ready for the writer
    bool stop = false;
    int64_t n_internal = 0;
    std::thread solver([&] {
        for (int k = 0; k < n_chunks; k++) {
            { std::lock_guard<std::mutex> lk(mu); if (stop) break; }
            const auto a0 = clk::now();
            std::memset(&outs[k], 0, sizeof(outs[k]));
            rcs[k] = aasm_solve_batch_range(&run.view, cut[k], cut[k + 1], &run.cli.opts, &outs[k]);
            const aasm_stats &st = outs[k].stats;
            if (rcs[k] != AASM_OK) errs[k] = aasm_last_error();
            else { tm.upload_s += st.reserved_f[0] / 1e3; tm.device_s += st.reserved_f[2] / 1e3; tm.fetch_s += st.reserved_f[1] / 1e3; n_internal += st.n_internal_errors; }
            tm.solve_busy_s += secs(a0, clk::now());
            { std::lock_guard<std::mutex> lk(mu); solved = k + 1; }
            cv.notify_all();
            if (rcs[k] != AASM_OK) break;
        }
    });
    int wrc = AASM_OK, src = AASM_OK;
    std::string fail;
    for (int k = 0; k < n_chunks; k++) {
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return solved > k; }); }
        if (rcs[k] != AASM_OK) { src = rcs[k]; fail = errs[k]; break; }
        if (k == n_chunks - 1) tm.t2 = clk::now();
        if (k == 0) std::cout << "Write output PAF file" << std::endl;          // :487
        const auto a0 = clk::now();
        wrc = aasm_writer_append(wr, run.paf, &outs[k], cut[k]);
        tm.write_busy_s += secs(a0, clk::now());
        if (wrc != AASM_OK) { fail = aasm_last_error(); break; }
    }
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    solver.join();
    const int crc = aasm_writer_close(wr, src == AASM_OK && wrc == AASM_OK ? 1 : 0);
    if (src == AASM_E_PARSE) return bad_input(fail);                            // malformed cs tag, found by the device parser
    if (src != AASM_OK) return solver_failed(src, fail);
    report_internal(n_internal);
    const int rc = wrc != AASM_OK ? wrc : crc;
    if (rc != AASM_OK) write_failed(wrc != AASM_OK ? fail : std::string(aasm_last_error()));
    return {Outcome::Written, rc};
}

// ---- 5: one piece, over cli.gpus GPUs
static Outcome route_one_piece(Run &run) {
    Timing &tm = run.tm;
    aasm_batch_out out;
    const int rc = aasm_solve_batch_multi(&run.view, &run.cli.opts, run.cli.gpus, &out);
    tm.t2 = clk::now();
    if (rc == AASM_E_PARSE) return bad_input(aasm_last_error());                // malformed cs tag, found by the device parser
    if (rc != AASM_OK) return solver_failed(rc, aasm_last_error());
    tm.upload_s = out.stats.reserved_f[0] / 1e3; tm.device_s = out.stats.reserved_f[2] / 1e3; tm.fetch_s = out.stats.reserved_f[1] / 1e3;
    tm.solve_busy_s = secs(tm.t1, tm.t2);
    return write_outputs(run, out);
}

int main(int argc, char **argv) {
    Cli cli;
    if (const int code = parse_args(argc, argv, cli); code >= 0) return code;
    Run run(cli);
    run.warm_up();
    Outcome o{Outcome::GoOn, AASM_OK};
    bool device_reader = cli.device_reader, device_writer = cli.device_writer;
    if (device_reader && device_writer && (!cli.use_alt || cli.device_alt) && cli.gpus <= 1) {
        o = route_no_container(run);
        device_reader = device_writer = false;                                  // done; or on with the host reader, as the command without the two flags
    }
    if (o.kind == Outcome::GoOn) o = read_container(run, device_reader);
    if (o.kind == Outcome::GoOn && device_writer) o = route_device_writer(run);
    if (o.kind == Outcome::GoOn && run.up) o = route_resident(run);
    if (o.kind == Outcome::GoOn) o = ranges_apply(run) ? route_ranges(run) : route_one_piece(run);
    if (o.kind == Outcome::Fatal) return o.rc;                                  // (~Run waits for the warm-up threads)
    if (cli.timing) print_timing(run.tm);
    // the process ends here: the GBs of parsed text and results go back to the OS in one piece
    // instead of vector by vector (1.7 s of page freeing for a 5M-record file)
    std::cout.flush(); std::cerr.flush();
    run.join_warm();
    std::_Exit(o.rc == AASM_OK ? 0 : 3);
}
