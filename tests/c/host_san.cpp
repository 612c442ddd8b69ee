// host_san -- stand-alone driver of the host stages (reader, input discovery, packer, forecast sink, model blobs,
// cross-validation plan) for sanitizer builds: tests/test_host_sanitize.py compiles this file together with
// csrc/tsf_csv.cpp, tsf_pack.cpp and tsf_cv_plan.cpp -- no HIP, no libtsf_amd.so, no Python -- once plainly, once with
// -fsanitize=address,undefined and once with -fsanitize=thread, runs every sub-command and compares what they dump.
//
//   host_san selfcheck heap|overflow|race      one planted host-only defect: the sanitizer must report it
//   host_san read   OUT dtq|sdtq FILE...       every file alone and all together; both modes; 1 and 4 threads
//   host_san pack   OUT CASES                  the cases of CASES (written by the test) through tsf_pack_rows_typed
//   host_san tree   OUT ROOT [fork]            discovery / load / chunked load of a Hive tree, alone and from two threads
//   host_san treeerr OUT DIR                   the error paths of discovery (DIR prepared by the test)
//   host_san sink   OUT DIR                    both widths of the forecast sink into DIR
//   host_san blobs  OUT                        tsf_model_blobs
//   host_san cvplan OUT                        tsf_cv_plan
//
// OUT is a sequence of records: 16 bytes of tag, int64 byte count, bytes (little-endian arrays as they lie in memory).
// Exit status: 0 fine, 2 usage / io, 3 a self-consistency check of the driver failed (message on stderr).
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "tsf.h"

namespace {

typedef std::string Blob;

void put(Blob &o, const char *tag, const void *p, size_t n) {
    char t[16] = {0};
    std::strncpy(t, tag, 15);
    const int64_t k = (int64_t)n;
    o.append(t, 16);
    o.append((const char *)&k, 8);
    if (n) o.append((const char *)p, n);
}
template <class T>
void putv(Blob &o, const char *tag, const std::vector<T> &v) { put(o, tag, v.data(), v.size() * sizeof(T)); }
void puti(Blob &o, const char *tag, std::initializer_list<int64_t> v) {
    std::vector<int64_t> x(v);
    putv(o, tag, x);
}

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "host_san: self-check failed: %s\n", what);
    std::exit(3);
}
#define CHECK(c) do { if (!(c)) fail(#c); } while (0)

bool save(const char *path, const Blob &b) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = b.empty() || std::fwrite(b.data(), 1, b.size(), f) == b.size();
    return std::fclose(f) == 0 && ok;
}

// ---- selfcheck ---------------------------------------------------------------------------------------------------
int racy_counter = 0;

int selfcheck(const char *which) {
    if (!std::strcmp(which, "heap")) {
        volatile size_t n = 16;
        char *p = new char[n];
        std::memset(p, 1, n);
        volatile char c = p[n];                 // one past the end
        delete[] p;
        return c == 77 ? 1 : 0;
    }
    if (!std::strcmp(which, "overflow")) {
        volatile int64_t x = std::numeric_limits<int64_t>::max();
        volatile int64_t y = x + 1;             // signed overflow
        return y == 77 ? 1 : 0;
    }
    if (!std::strcmp(which, "race")) {
        auto f = [] { for (int i = 0; i < 200000; ++i) racy_counter = racy_counter + 1; };    // no synchronisation
        std::thread a(f), b(f);
        a.join();
        b.join();
        return racy_counter == 77 ? 1 : 0;
    }
    return 2;
}

// ---- reader ------------------------------------------------------------------------------------------------------
// one table (or error) as a record group: head = rc, err_file, err_line, malformed, n_rows
void dump_table(Blob &o, int rc, tsf_csv *t, int64_t n_rows, int32_t ef, int64_t el) {
    if (rc != 0) {
        CHECK(t == nullptr);
        puti(o, "head", {rc, ef, el, -1, 0});
        return;
    }
    CHECK(t != nullptr);
    const size_t n = (size_t)n_rows;
    std::vector<int64_t> sid(n + 1), did(n + 1), ds(n + 1);
    std::vector<double> y(n + 1);
    const int64_t *csid, *cdid, *cds;
    const double *cy;
    CHECK(tsf_csv_columns(t, &csid, &cdid, &cds, &cy) == 0);
    CHECK(tsf_csv_fetch(t, sid.data(), did.data(), ds.data(), y.data()) == 0);
    CHECK(tsf_csv_fetch(t, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(!n || (!std::memcmp(csid, sid.data(), n * 8) && !std::memcmp(cdid, did.data(), n * 8) &&
                 !std::memcmp(cds, ds.data(), n * 8) && !std::memcmp(cy, y.data(), n * 8)));
    puti(o, "head", {rc, ef, el, tsf_csv_malformed(t), n_rows});
    put(o, "sid", sid.data(), n * 8);
    put(o, "did", did.data(), n * 8);
    put(o, "ds", ds.data(), n * 8);
    put(o, "y", y.data(), n * 8);
    tsf_csv_free(t);
}

void read_once(Blob &o, int n, const char *const *paths, const int64_t *sids, const char *layout, int nt) {
    tsf_csv *t = nullptr;
    int64_t n_rows = 0, el = 0;
    int32_t ef = -1;
    const int rc = tsf_csv_read(n, paths, sids, layout, nt, &t, &n_rows, &ef, &el);
    dump_table(o, rc, t, n_rows, ef, el);
}

int cmd_read(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::string base = argv[3];
    const bool has_s = base.find('s') != std::string::npos;
    // files after a "--" are read alone only (streams that cannot be opened would fail every call that lists them)
    std::vector<const char *> paths;
    int n = 0;
    for (int i = 4; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--")) { n = (int)paths.size(); continue; }
        paths.push_back(argv[i]);
    }
    const int n_all = (int)paths.size();
    if (n == 0) n = n_all;
    std::vector<int64_t> sids((size_t)n_all);
    for (int i = 0; i < n_all; ++i) sids[(size_t)i] = 1000 + i;
    Blob o;
    for (const std::string &lay : {base, base + "?"})
        for (int nt : {1, 4}) {
            for (int i = 0; i < n_all; ++i) read_once(o, 1, &paths[(size_t)i], has_s ? nullptr : &sids[(size_t)i], lay.c_str(), nt);
            read_once(o, n, paths.data(), has_s ? nullptr : sids.data(), lay.c_str(), nt);
        }
    // bad arguments come back as -1 and leave nothing behind
    tsf_csv *t = nullptr;
    CHECK(tsf_csv_read(n, paths.data(), sids.data(), "dq", 1, &t, nullptr, nullptr, nullptr) == -1 && !t);
    CHECK(tsf_csv_read(n, paths.data(), nullptr, "dtq", 1, &t, nullptr, nullptr, nullptr) == (n > 0 ? -1 : 0));
    if (t) tsf_csv_free(t);
    tsf_csv_free(nullptr);
    return save(argv[2], o) ? 0 : 2;
}

// ---- packer ------------------------------------------------------------------------------------------------------
struct Fetched {
    std::vector<int64_t> ksid, kdid, off, ds, span, mdt;
    std::vector<double> y, ymax;
    int32_t flags[4];
};

int cmd_pack(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = std::fopen(argv[3], "rb");
    if (!f) return 2;
    Blob o;
    for (;;) {
        int64_t head[3];                        // n, key_bytes, y_dtype
        if (std::fread(head, 8, 3, f) != 3) break;
        const int64_t n = head[0];
        const int kb = (int)head[1], ydt = (int)head[2], yb = ydt == TSF_Y_F64 ? 8 : 4;
        // (exact sizes, so that a read past the end of an input is a read past the end of its allocation)
        std::vector<char> sid((size_t)(n * kb)), did((size_t)(n * kb)), y((size_t)(n * yb));
        std::vector<int64_t> ds((size_t)n);
        if ((n > 0) && (std::fread(sid.data(), (size_t)kb, (size_t)n, f) != (size_t)n || std::fread(did.data(), (size_t)kb, (size_t)n, f) != (size_t)n ||
                        std::fread(ds.data(), 8, (size_t)n, f) != (size_t)n || std::fread(y.data(), (size_t)yb, (size_t)n, f) != (size_t)n))
            return 2;
        for (int nt : {1, 4}) {
            tsf_pack *p = nullptr;
            int64_t R = -1, NS = -1;
            int32_t ident = -1;
            const int rc = tsf_pack_rows_typed(n, sid.data(), did.data(), kb, ds.data(), y.data(), ydt, nt, &p, &R, &NS, &ident);
            puti(o, "pack", {rc, R, NS, ident});
            if (rc != 0) continue;
            int32_t fl[4];
            CHECK(tsf_pack_flags(p, fl, fl + 1, fl + 2, fl + 3) == -1);        // not before a fetch
            Fetched full;
            auto fetch = [&](Fetched &g, unsigned null_mask) {
                g.ksid.assign((size_t)NS, -7); g.kdid.assign((size_t)NS, -7); g.off.assign((size_t)NS + 1, -7);
                g.ds.assign((size_t)R, -7); g.y.assign((size_t)R, -7.0);
                g.span.assign((size_t)NS, -7); g.mdt.assign((size_t)NS, -7); g.ymax.assign((size_t)NS, -7.0);
                auto sel = [&](int bit, auto *ptr) { return (null_mask >> bit) & 1u ? nullptr : ptr; };
                CHECK(tsf_pack_fetch(p, sel(0, g.ksid.data()), sel(1, g.kdid.data()), sel(2, g.off.data()), sel(3, g.ds.data()),
                                     sel(4, g.y.data()), sel(5, g.span.data()), sel(6, g.mdt.data()), sel(7, g.ymax.data())) == 0);
                CHECK(tsf_pack_flags(p, g.flags, g.flags + 1, g.flags + 2, g.flags + 3) == 0);
            };
            fetch(full, 0);
            // every output NULL in turn: the others come out the same, and so do the flags
            for (int bit = 0; bit < 8; ++bit) {
                Fetched g;
                fetch(g, 1u << bit);
                auto same = [&](int b, const auto &u, const auto &v) {
                    return b == bit || u.empty() || !std::memcmp(u.data(), v.data(), u.size() * sizeof(u[0]));
                };
                CHECK(same(0, g.ksid, full.ksid) && same(1, g.kdid, full.kdid) && same(2, g.off, full.off) && same(3, g.ds, full.ds));
                CHECK(same(4, g.y, full.y) && same(5, g.span, full.span) && same(6, g.mdt, full.mdt) && same(7, g.ymax, full.ymax));
                CHECK(!std::memcmp(g.flags, full.flags, sizeof(g.flags)));
            }
            tsf_pack_free(p);
            {
                // in place, on a copy of the table: ds_out is the ds array the plan was built from (and y_out the y array
                // where that is f64)
                std::vector<int64_t> ds2(ds);
                std::vector<char> y2(y);
                tsf_pack *q = nullptr;
                CHECK(tsf_pack_rows_typed(n, sid.data(), did.data(), kb, ds2.data(), y2.data(), ydt, nt, &q, nullptr, nullptr, nullptr) == 0);
                CHECK(tsf_pack_fetch(q, nullptr, nullptr, nullptr, ds2.data(), ydt == TSF_Y_F64 ? (double *)y2.data() : nullptr,
                                     nullptr, nullptr, nullptr) == 0);
                CHECK(R == 0 || !std::memcmp(ds2.data(), full.ds.data(), (size_t)R * 8));
                CHECK(R == 0 || ydt != TSF_Y_F64 || !std::memcmp(y2.data(), full.y.data(), (size_t)R * 8));
                tsf_pack_free(q);
            }
            putv(o, "ksid", full.ksid); putv(o, "kdid", full.kdid); putv(o, "off", full.off);
            putv(o, "ds", full.ds); putv(o, "y", full.y);
            putv(o, "span", full.span); putv(o, "min_dt", full.mdt); putv(o, "y_max", full.ymax);
            put(o, "flags", full.flags, sizeof(full.flags));
        }
    }
    std::fclose(f);
    tsf_pack *p = nullptr;
    CHECK(tsf_pack_rows_typed(1, nullptr, nullptr, 8, nullptr, nullptr, TSF_Y_F64, 1, &p, nullptr, nullptr, nullptr) == -1);
    int64_t one = 1;
    double yy = 1;
    CHECK(tsf_pack_rows_typed(1, &one, &one, 2, &one, &yy, TSF_Y_F64, 1, &p, nullptr, nullptr, nullptr) == -1);
    CHECK(tsf_pack_fetch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    tsf_pack_free(nullptr);
    return save(argv[2], o) ? 0 : 2;
}

// ---- discovery ---------------------------------------------------------------------------------------------------
void dump_dir(Blob &o, const char *root, int rc, tsf_csv_dir *d, int32_t nf, int32_t np) {
    puti(o, "dir", {rc, nf, np});
    if (!d) return;
    const char *const *paths = tsf_csv_dir_paths(d);
    const int64_t *sids = tsf_csv_dir_series_id(d);
    const size_t skip = std::strlen(root);
    std::string names;
    for (int32_t i = 0; i < nf; ++i) {
        const char *p = paths[i];
        names += (std::strncmp(p, root, skip) == 0 ? p + skip : p);       // relative: the same bytes wherever the tree lies
        names += '\n';
    }
    put(o, "paths", names.data(), names.size());
    put(o, "sids", sids, (size_t)nf * 8);
    const char *ep = tsf_csv_dir_error_path(d);
    const std::string e = std::strncmp(ep, root, skip) == 0 ? ep + skip : ep;
    put(o, "err_path", e.data(), e.size());
}

void read_loaded(Blob &o, tsf_csv_dir *d, int32_t first, int32_t count, const char *layout, int nt) {
    tsf_csv *t = nullptr;
    int64_t n_rows = 0, el = 0;
    int32_t ef = -1;
    const int rc = tsf_csv_read_loaded(d, first, count, layout, nt, &t, &n_rows, &ef, &el);
    dump_table(o, rc, t, n_rows, ef, el);
}

// the successful paths over one tree with `nt` threads: list + read, list-and-load + read, the root in ranges
Blob tree_pass(const char *root, int nt) {
    Blob o;
    tsf_csv_dir *d = nullptr;
    int32_t nf = 0, np = 0;
    int rc = tsf_csv_discover(root, nt, &d, &nf, &np);
    dump_dir(o, root, rc, d, nf, np);
    CHECK(rc == 0 && d);
    read_once(o, np, tsf_csv_dir_paths(d), tsf_csv_dir_series_id(d), "dtq", nt);
    read_once(o, nf - np, tsf_csv_dir_paths(d) + np, nullptr, "sdtq?", nt);
    tsf_csv *t = nullptr;
    CHECK(tsf_csv_read_loaded(d, 0, nf, "dtq", nt, &t, nullptr, nullptr, nullptr) == -1);     // not a preloaded handle
    tsf_csv_dir_free(d);

    d = nullptr;
    rc = tsf_csv_discover_load(root, nt, &d, &nf, &np);
    dump_dir(o, root, rc, d, nf, np);
    CHECK(rc == 0 && d);
    CHECK(tsf_csv_read_loaded(d, 0, nf + 1, "dtq", nt, &t, nullptr, nullptr, nullptr) == -1);
    read_loaded(o, d, 0, np / 2, "dtq?", nt);
    read_loaded(o, d, np / 2, np - np / 2, "dtq", nt);
    read_loaded(o, d, np, nf - np, "sdtq?", nt);
    read_loaded(o, d, 0, 0, "dtq", nt);
    tsf_csv_dir_free(d);
    // (a loaded handle dropped unread gives its arenas back too)
    d = nullptr;
    CHECK(tsf_csv_discover_load(root, nt, &d, &nf, &np) == 0);
    tsf_csv_dir_free(d);

    tsf_csv_root *r = nullptr;
    int32_t nc = 0, hive = -1;
    rc = tsf_csv_root_open(root, &r, &nc, &hive);
    puti(o, "root", {rc, nc, hive});
    CHECK(rc == 0 && r);
    const int32_t cuts[5] = {0, 0, nc / 3, nc - 1 > 0 ? nc - 1 : 0, nc};      // [0, 0) first: a range of no children
    for (int k = 0; k + 1 < 5; ++k) {
        const int32_t first = cuts[k], count = cuts[k + 1] - cuts[k];
        int32_t nested = -1;
        d = nullptr;
        rc = tsf_csv_root_load(r, first, count, nt, &d, &nf, &np, &nested);
        dump_dir(o, root, rc, d, nf, np);
        puti(o, "nested", {nested});
        CHECK(rc == 0 && d);
        read_loaded(o, d, 0, np, "dtq?", nt);
        read_loaded(o, d, np, nf - np, "sdtq?", nt);
        tsf_csv_dir_free(d);
    }
    d = nullptr;
    CHECK(tsf_csv_root_load(r, 0, nc + 1, nt, &d, nullptr, nullptr, nullptr) == -1);
    tsf_csv_root_free(r);
    return o;
}

int cmd_tree(int argc, char **argv) {
    if (argc < 4) return 2;
    const char *root = argv[3];
    const bool with_fork = argc > 4 && !std::strcmp(argv[4], "fork");
    const Blob alone = tree_pass(root, 4);
    Blob a, b;
    {
        std::thread ta([&] { a = tree_pass(root, 2); }), tb([&] { b = tree_pass(root, 5); });
        ta.join();
        tb.join();
    }
    CHECK(a == alone && b == alone);
    if (with_fork) {
        // the pool has started: a forked child has none of its threads and must start its own
        std::fflush(nullptr);
        const pid_t pid = fork();
        if (pid < 0) return 2;
        if (pid == 0) {
            const Blob c = tree_pass(root, 4);
            std::fflush(nullptr);
            _exit(c == alone ? 0 : 3);
        }
        int st = 0;
        CHECK(waitpid(pid, &st, 0) == pid);
        if (!(WIFEXITED(st) && WEXITSTATUS(st) == 0)) {
            std::fprintf(stderr, "host_san: forked child ended with status 0x%x\n", st);
            return 3;
        }
        CHECK(tree_pass(root, 4) == alone);
    }
    return save(argv[2], alone) ? 0 : 2;
}

// DIR holds: bad_sid/ (a series_id=abc directory), codec/ (a .snappy part), empty/ (nothing), noperm/ (a directory the
// test made unreadable, where it could), vanish/ (a file this program deletes between listing and reading), file.csv
int cmd_treeerr(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string base = argv[3];
    Blob o;
    for (const char *sub : {"/bad_sid", "/codec", "/empty", "/noperm", "/file.csv", "/missing"})
        for (int load = 0; load < 2; ++load) {
            const std::string root = base + sub;
            tsf_csv_dir *d = nullptr;
            int32_t nf = -1, np = -1;
            const int rc = (load ? tsf_csv_discover_load : tsf_csv_discover)(root.c_str(), 3, &d, &nf, &np);
            dump_dir(o, root.c_str(), rc, d, nf, np);
            if (d && load && rc == 0) read_loaded(o, d, 0, nf, nf == np ? "dtq?" : "sdtq?", 3);
            if (d && load && rc == TSF_CSV_E_CODEC) read_loaded(o, d, 0, nf, "dtq?", 3);       // the refused part was not loaded
            tsf_csv_dir_free(d);
            tsf_csv_root *r = nullptr;
            int32_t nc = -1, hive = -1;
            const int rr = tsf_csv_root_open(root.c_str(), &r, &nc, &hive);
            puti(o, "root", {rr, nc, hive});
            if (r) {
                int32_t nested = -1;
                d = nullptr;
                const int rl = tsf_csv_root_load(r, 0, nc, 3, &d, &nf, &np, &nested);
                dump_dir(o, root.c_str(), rl, d, nf, np);
                tsf_csv_dir_free(d);
                tsf_csv_root_free(r);
            }
        }
    {
        const std::string root = base + "/vanish";
        tsf_csv_dir *d = nullptr;
        int32_t nf = 0, np = 0;
        CHECK(tsf_csv_discover(root.c_str(), 2, &d, &nf, &np) == 0 && nf == 3 && np == 3);
        CHECK(::unlink(tsf_csv_dir_paths(d)[1]) == 0);
        read_once(o, nf, tsf_csv_dir_paths(d), tsf_csv_dir_series_id(d), "dtq?", 2);     // TSF_CSV_E_OPEN, err_file 1
        tsf_csv_dir_free(d);
    }
    tsf_csv_dir *d = nullptr;
    CHECK(tsf_csv_discover(nullptr, 1, &d, nullptr, nullptr) == -1);
    CHECK(tsf_csv_dir_paths(nullptr) == nullptr && tsf_csv_dir_series_id(nullptr) == nullptr);
    tsf_csv_dir_free(nullptr);
    tsf_csv_root_free(nullptr);
    return save(argv[2], o) ? 0 : 2;
}

// ---- sink and blobs ----------------------------------------------------------------------------------------------
uint64_t lcg(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 11; }

Blob slurp(const std::string &path) {
    Blob b;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) fail("sink output missing");
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) b.append(buf, k);
    std::fclose(f);
    return b;
}

int cmd_sink(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string dir = argv[3];
    const int64_t I64_MIN = std::numeric_limits<int64_t>::min(), I64_MAX = std::numeric_limits<int64_t>::max();
    const int32_t I32_MIN = std::numeric_limits<int32_t>::min(), I32_MAX = std::numeric_limits<int32_t>::max();
    Blob o;
    uint64_t seed = 13;
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)9001}) {          // 9001 rows: three blocks of 4 096, several threads
        std::vector<int64_t> s64((size_t)n), d64((size_t)n), q64((size_t)n), ds((size_t)n);
        std::vector<int32_t> s32((size_t)n), d32((size_t)n), q32((size_t)n);
        const int64_t ext_ds[6] = {I64_MIN, I64_MAX, -1, 0, -86400000000000ll, 86399999999999ll};
        const int64_t ext_id[4] = {I64_MIN, I64_MAX, 0, -1};
        for (int64_t i = 0; i < n; ++i) {
            const size_t k = (size_t)i;
            const uint64_t hi = lcg(seed), lo = lcg(seed) & 0x7ff;
            ds[k] = i < 6 ? ext_ds[i] : (int64_t)(hi << 11 | lo);
            s64[k] = i < 4 ? ext_id[i] : (int64_t)lcg(seed) - ((int64_t)1 << 52);
            d64[k] = i < 4 ? ext_id[3 - i] : (int64_t)(lcg(seed) % 1000);
            q64[k] = i < 4 ? ext_id[(i + 1) % 4] : (int64_t)lcg(seed) - ((int64_t)1 << 52);
            s32[k] = i == 0 ? I32_MIN : (i == 1 ? I32_MAX : (int32_t)(lcg(seed) & 0xffffffffu));
            d32[k] = (int32_t)(lcg(seed) % 1000);
            q32[k] = i == 0 ? I32_MAX : (i == 1 ? I32_MIN : (int32_t)(lcg(seed) & 0xffffffffu));
        }
        if (n == 1) ds[0] = I64_MIN;
        for (int nt : {1, 5}) {
            const std::string p64 = dir + "/f64_" + std::to_string(n) + "_" + std::to_string(nt) + ".csv";
            const std::string p32 = dir + "/f32_" + std::to_string(n) + "_" + std::to_string(nt) + ".csv";
            CHECK(tsf_csv_write_forecasts(p64.c_str(), "2020-01-01T00:00:00+00:00", n, s64.data(), d64.data(), ds.data(), q64.data(), nt) == 0);
            CHECK(tsf_csv_write_forecasts_i32(p32.c_str(), "", n, s32.data(), d32.data(), ds.data(), q32.data(), nt) == 0);
            const Blob a = slurp(p64), b = slurp(p32);
            put(o, "csv64", a.data(), a.size());
            put(o, "csv32", b.data(), b.size());
        }
        const std::string nowhere = dir + "/no/such/dir/out.csv";
        CHECK(tsf_csv_write_forecasts(nowhere.c_str(), "x", n, s64.data(), d64.data(), ds.data(), q64.data(), 2) == TSF_CSV_E_OPEN);
        CHECK(tsf_csv_write_forecasts_i32(nowhere.c_str(), "x", n, s32.data(), d32.data(), ds.data(), q32.data(), 2) == TSF_CSV_E_OPEN);
        CHECK(tsf_csv_write_forecasts((dir + "/x.csv").c_str(), nullptr, n, s64.data(), d64.data(), ds.data(), q64.data(), 2) == -1);
        const std::string longstamp(65, 'x');
        CHECK(tsf_csv_write_forecasts((dir + "/x.csv").c_str(), longstamp.c_str(), n, s64.data(), d64.data(), ds.data(), q64.data(), 2) == -1);
    }
    return save(argv[2], o) ? 0 : 2;
}

int cmd_blobs(int argc, char **argv) {
    if (argc != 3) return 2;
    Blob o;
    uint64_t seed = 29;
    const char prefix_bytes[] = "TSFM\x02{\"growth\":\"linear\"}";
    for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)2500})               // >= 2 048: the parallel path
        for (int per_series_grid = 0; per_series_grid < 2; ++per_series_grid)
            for (int32_t ntc : {0, TSF_MAX_S + 4})
                for (int32_t plen : {0, (int32_t)sizeof(prefix_bytes) - 1}) {
                    const int32_t n_grids = per_series_grid ? (int32_t)N : 1;
                    if (n_grids < 1) continue;                      // (N = 0 with one grid per series is no valid call)
                    const int32_t n_theta = 3 + (int32_t)(N % 7);
                    std::vector<double> theta((size_t)(N * n_theta)), ysc((size_t)N);
                    std::vector<int64_t> last((size_t)N);
                    std::vector<int32_t> status((size_t)N), iters((size_t)N);
                    std::vector<tsf_grid_info> grid((size_t)n_grids);
                    std::memset((void *)grid.data(), 0, grid.size() * sizeof(tsf_grid_info));
                    for (auto &g : grid) {
                        g.start_ns = (int64_t)lcg(seed); g.t_scale_ns = (int64_t)lcg(seed) + 1;
                        g.T = (int32_t)(lcg(seed) % 5000); g.S = (int32_t)(lcg(seed) % 25); g.i1 = 3; g.NT = g.T;
                        for (int k = 0; k < TSF_MAX_S + 4; ++k) g.t_change[k] = (double)(lcg(seed) % 1000) / 1000.0;
                    }
                    for (auto &v : theta) v = (double)(int64_t)(lcg(seed) % 2001 - 1000) / 64.0;
                    for (int64_t i = 0; i < N; ++i) {
                        ysc[(size_t)i] = (double)(lcg(seed) % 100000) / 8.0;
                        last[(size_t)i] = (int64_t)lcg(seed);
                        status[(size_t)i] = (int32_t)(lcg(seed) % 64) - 8;
                        iters[(size_t)i] = (int32_t)(lcg(seed) % 10000);
                    }
                    const size_t stride = (size_t)plen + 64 + 8 * ((size_t)n_theta + (size_t)ntc);
                    Blob first;
                    for (int nt : {1, 6}) {
                        std::vector<char> out((size_t)N * stride);      // exact: a write past the end is a heap overflow
                        CHECK(tsf_model_blobs(N, prefix_bytes, plen, n_theta, theta.data(), ysc.data(), grid.data(), n_grids, last.data(),
                                              status.data(), iters.data(), ntc, out.data(), nt) == 0);
                        const Blob b(out.data(), out.size());
                        if (nt == 1) first = b;
                        CHECK(b == first);
                    }
                    puti(o, "blobs", {N, n_grids, ntc, plen, n_theta});
                    put(o, "bytes", first.data(), first.size());
                }
    double x = 0;
    CHECK(tsf_model_blobs(1, nullptr, 0, 1, &x, &x, nullptr, 1, nullptr, nullptr, nullptr, 0, &x, 1) == -1);
    CHECK(tsf_model_blobs(0, nullptr, 0, 1, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, TSF_MAX_S + 5, nullptr, 1) == -1);
    CHECK(tsf_model_blobs(0, nullptr, 0, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, 0, nullptr, 1) == 0);
    return save(argv[2], o) ? 0 : 2;
}

// ---- cross-validation plan ---------------------------------------------------------------------------------------
void plan_once(Blob &o, int64_t N, int32_t T, const std::vector<int64_t> *offsets, const std::vector<int64_t> &ds, tsf_cv_args a) {
    std::vector<int32_t> nfolds((size_t)N), status((size_t)N);
    std::vector<int64_t> nh((size_t)N), nm((size_t)N);
    // sized first without the per-fold outputs, then exactly
    int rc = tsf_cv_plan(N, T, offsets ? offsets->data() : nullptr, ds.data(), &a, nfolds.data(), status.data(), nh.data(), nm.data(),
                         nullptr, nullptr, nullptr);
    puti(o, "cvplan", {rc, N, T});
    if (rc != 0) return;
    int64_t F = 0;
    for (int32_t k : nfolds) F += k;
    std::vector<int64_t> cutoff((size_t)F);
    std::vector<int32_t> hist((size_t)F), hold((size_t)F);
    CHECK(tsf_cv_plan(N, T, offsets ? offsets->data() : nullptr, ds.data(), &a, nfolds.data(), status.data(), nh.data(), nm.data(),
                      cutoff.data(), hist.data(), hold.data()) == 0);
    putv(o, "n_folds", nfolds); putv(o, "status", status); putv(o, "n_holdout", nh); putv(o, "n_metric", nm);
    putv(o, "cutoff", cutoff); putv(o, "hist_rows", hist); putv(o, "hold_rows", hold);
}

int cmd_cvplan(int argc, char **argv) {
    if (argc != 3) return 2;
    const int64_t DAY = 86400000000000ll, T0 = 1546300800000000000ll;          // 2019-01-01
    Blob o;
    auto daily = [&](int64_t T, int64_t start) {
        std::vector<int64_t> v((size_t)T);
        for (int64_t i = 0; i < T; ++i) v[(size_t)i] = start + i * DAY;
        return v;
    };
    // aligned: 730 daily rows, horizon 90 d, the defaults (test_default_period_and_initial_cfg2_shape), then explicit ones
    plan_once(o, 4, 730, nullptr, daily(730, T0), tsf_cv_args{90 * DAY, 0, -1, 0.1});
    for (auto pi : {std::pair<int, int>{7, 30}, {30, 0}, {45, 400}, {200, 100}, {1, 700}})
        plan_once(o, 1, 730, nullptr, daily(730, T0), tsf_cv_args{60 * DAY, pi.first * DAY, pi.second * DAY, 0.1});
    // the statuses (test_error_statuses): less data than the horizon, no cutoff after the initial window, too few rows
    plan_once(o, 1, 20, nullptr, daily(20, T0), tsf_cv_args{30 * DAY, 0, -1, 0.1});
    plan_once(o, 1, 100, nullptr, daily(100, T0), tsf_cv_args{30 * DAY, 0, -1, 0.1});
    plan_once(o, 2, 1, nullptr, daily(1, T0), tsf_cv_args{DAY, 0, -1, 1.0});
    // ragged: the 120-day hole (test_gap_triggers_closest_date_jump), an empty series, a one-row series, a series
    // shorter than the horizon, one row before a long gap, duplicate timestamps
    std::vector<int64_t> ds, off(1, 0);
    auto add = [&](const std::vector<int64_t> &v) { ds.insert(ds.end(), v.begin(), v.end()); off.push_back((int64_t)ds.size()); };
    {
        std::vector<int64_t> g = daily(800, T0);
        g.erase(g.begin() + 300, g.begin() + 420);
        add(g);
    }
    add({});
    add(daily(1, T0));
    add(daily(12, T0));
    {
        std::vector<int64_t> g = daily(1, T0 - 365 * DAY), h = daily(200, T0);
        g.insert(g.end(), h.begin(), h.end());
        add(g);
    }
    {
        std::vector<int64_t> g;
        for (int64_t i = 0; i < 300; ++i) { g.push_back(T0 + (i / 2) * DAY + 40500000000000ll); }
        add(g);
    }
    const int64_t N = (int64_t)off.size() - 1;
    for (double rw : {0.0, 0.1, 0.25, 1.0})
        for (auto pi : {std::pair<int, int>{20, 60}, {5, 60}, {13, 0}, {100, 90}, {0, -1}})
            plan_once(o, N, 0, &off, ds, tsf_cv_args{30 * DAY, pi.first * DAY, pi.second * DAY, rw});
    // bad arguments
    tsf_cv_args bad{0, 0, -1, 0.1};
    std::vector<int32_t> a((size_t)N), b((size_t)N);
    std::vector<int64_t> c((size_t)N), d((size_t)N);
    CHECK(tsf_cv_plan(N, 0, off.data(), ds.data(), &bad, a.data(), b.data(), c.data(), d.data(), nullptr, nullptr, nullptr) == -1);
    bad = tsf_cv_args{DAY, 0, -1, 1.5};
    CHECK(tsf_cv_plan(N, 0, off.data(), ds.data(), &bad, a.data(), b.data(), c.data(), d.data(), nullptr, nullptr, nullptr) == -1);
    bad = tsf_cv_args{DAY, 0, -1, 0.5};
    CHECK(tsf_cv_plan(N, 5, off.data(), ds.data(), &bad, a.data(), b.data(), c.data(), d.data(), nullptr, nullptr, nullptr) == -1);
    CHECK(tsf_cv_plan(0, 0, off.data(), ds.data(), &bad, a.data(), b.data(), c.data(), d.data(), nullptr, nullptr, nullptr) == -1);
    return save(argv[2], o) ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: host_san selfcheck|read|pack|tree|treeerr|sink|blobs|cvplan ...\n");
        return 2;
    }
    const std::string cmd = argv[1];
    if (cmd == "selfcheck") return selfcheck(argv[2]);
    if (cmd == "read") return cmd_read(argc, argv);
    if (cmd == "pack") return cmd_pack(argc, argv);
    if (cmd == "tree") return cmd_tree(argc, argv);
    if (cmd == "treeerr") return cmd_treeerr(argc, argv);
    if (cmd == "sink") return cmd_sink(argc, argv);
    if (cmd == "blobs") return cmd_blobs(argc, argv);
    if (cmd == "cvplan") return cmd_cvplan(argc, argv);
    return 2;
}
