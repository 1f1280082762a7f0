// test_pssm_tables -- build_pssm_tables (lightmotif_amd/csrc/pssm_tables.hpp) on the CPU: the device image of a scoring
// matrix against digests recorded from the code it replaced (tests/golden/pssm_tables_digest.json: presence, size and
// 64-bit FNV-1a of every table, and the scalars the launch code reads), and the layout of the image itself -- every table
// on a 256-byte boundary, none overlapping, all inside `bytes`, zero padding, slices that tile [0, m).
//   usage: test_pssm_tables <tests/golden/pssm_tables_digest.json>
// The matrices come from an integer LCG scaled by a power of two (no libm, no RNG library); the last column (N / X) is -inf.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <string>

#include "pssm_tables.hpp"

using namespace lm;

// ---- the matrices ------------------------------------------------------------------------------------------------------

static const size_t kLengths[] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                                  18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                                  35, 36, 37, 40, 44, 63, 64, 65, 72, 73, 88, 89, 100, 128, 129, 200};
static const size_t kAlphabets[] = {4, 5, 16, 17, 21, 64, 65};
static const char *const kSpecials[] = {"nan", "pinf", "ninf_row", "no_spread", "below_limit", "above_limit"};

static float from_bits(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t to_bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static const float kNegInf = from_bits(0xff800000u), kPosInf = from_bits(0x7f800000u), kNaN = from_bits(0x7fc00000u);

// weights in (-8, 8) on a grid of 2^-12
static std::vector<float> make_matrix(size_t m, size_t k)
{
    uint64_t state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)m << 32) ^ (uint64_t)k;
    std::vector<float> w(m * k);
    for (size_t j = 0; j < m; ++j)
        for (size_t s = 0; s < k; ++s) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            w[j * k + s] = s + 1 == k ? kNegInf : (float)((int)((state >> 40) & 0xffff) - 32768) * (1.0f / 4096.0f);
        }
    return w;
}

// m = 20, k = 5: the edges of the prefilter's conditions
static std::vector<float> make_special(const std::string &what)
{
    const size_t m = 20, k = 5;
    std::vector<float> w = make_matrix(m, k);
    if (what == "nan")
        w[7 * k + 2] = kNaN;
    else if (what == "pinf")
        w[11 * k + 1] = kPosInf;
    else if (what == "ninf_row")
        for (size_t s = 0; s < k; ++s)
            w[5 * k + s] = kNegInf;
    else if (what == "no_spread")
        for (size_t j = 0; j < m; ++j)
            for (size_t s = 0; s + 1 < k; ++s)
                w[j * k + s] = w[j * k];
    else {
        // every row's largest |w| is x, x the greatest float with 20 x (1 + 21 * 2^-23) < FLT_MAX; "above_limit" raises the
        // last row's by one ulp at a time until the sum reaches the limit.  (20 floats of one exponent add up exactly in double.)
        const double f = 1.0 + 21.0 / 8388608.0, flt_max = (double)from_bits(0x7f7fffffu);
        float x = (float)(flt_max / f / 20.0);
        while (20.0 * (double)x * f >= flt_max)
            x = from_bits(to_bits(x) - 1);
        float last = x;
        if (what == "above_limit")
            while ((19.0 * (double)x + (double)last) * f < flt_max)
                last = from_bits(to_bits(last) + 1);
        for (size_t j = 0; j < m; ++j)
            w[j * k + j % 4] = (j % 2 ? -1.0f : 1.0f) * (j + 1 == m ? last : x);
    }
    return w;
}

// ---- digests -----------------------------------------------------------------------------------------------------------

struct Sub {
    std::string name;
    const unsigned char *p;  // nullptr: the matrix has no such table
    size_t n;
};
struct Scalars {
    size_t ts = 0, lead = 0;
    std::vector<PssmTables::Part> parts;  // `table` is not part of the digest
    unsigned drop_dmax = 0;
    bool has_prefilter = false;
    double pre_offset = 0, pre_factor = 0, pre_emax = 0;
};

static uint64_t fnv1a(const unsigned char *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i)
        h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

static std::string hex_double(double d)
{
    uint64_t u;
    std::memcpy(&u, &d, 8);
    char buf[32];
    std::snprintf(buf, sizeof buf, "\"%016" PRIx64 "\"", u);
    return buf;
}

// One JSON object on one line; the recorded file holds exactly this text per case.
static std::string digest(const std::vector<Sub> &subs, const Scalars &sc)
{
    std::string out = "{\"tables\": {";
    char buf[160];
    for (size_t i = 0; i < subs.size(); ++i) {
        if (subs[i].p)
            std::snprintf(buf, sizeof buf, "\"%s\": [%zu, \"%016" PRIx64 "\"]", subs[i].name.c_str(), subs[i].n, fnv1a(subs[i].p, subs[i].n));
        else
            std::snprintf(buf, sizeof buf, "\"%s\": null", subs[i].name.c_str());
        out += (i ? ", " : "") + std::string(buf);
    }
    std::snprintf(buf, sizeof buf, "}, \"ts\": %zu, \"lead\": %zu, \"parts\": [", sc.ts, sc.lead);
    out += buf;
    for (size_t i = 0; i < sc.parts.size(); ++i) {
        std::snprintf(buf, sizeof buf, "%s[%zu, %zu, %zu, %zu]", i ? ", " : "", sc.parts[i].off, sc.parts[i].m, sc.parts[i].ts, sc.parts[i].lead);
        out += buf;
    }
    std::snprintf(buf, sizeof buf, "], \"drop_dmax\": %u, \"has_prefilter\": %s, ", sc.drop_dmax, sc.has_prefilter ? "true" : "false");
    out += buf;
    return out + "\"pre_offset\": " + hex_double(sc.pre_offset) + ", \"pre_factor\": " + hex_double(sc.pre_factor) + ", \"pre_emax\": " +
           hex_double(sc.pre_emax) + "}";
}

struct Case {
    std::string name;
    std::vector<float> w;
    size_t m, k;
    bool xlong_store;
};

static std::vector<Case> all_cases()
{
    std::vector<Case> cases;
    for (size_t m : kLengths)
        for (size_t k : kAlphabets)
            for (int x = 1; x >= (m > 64 ? 0 : 1); --x)
                cases.push_back({"m" + std::to_string(m) + "_k" + std::to_string(k) + (x ? "" : "_sliced"), make_matrix(m, k), m, k, x != 0});
    for (const char *what : kSpecials)
        cases.push_back({std::string("m20_k5_") + what, make_special(what), 20, 5, true});
    return cases;
}

// ---- the image of build_pssm_tables ------------------------------------------------------------------------------------

static int failures = 0;
#define CHECK(cond, ...)                                                                                                 \
    do {                                                                                                                 \
        if (!(cond)) {                                                                                                   \
            ++failures;                                                                                                  \
            std::fprintf(stderr, "FAIL %s: ", name.c_str());                                                             \
            std::fprintf(stderr, __VA_ARGS__);                                                                           \
            std::fprintf(stderr, "\n");                                                                                  \
        }                                                                                                                \
    } while (0)

// The tables of an image with the sizes their readers assume (the image itself records offsets only).
static std::vector<Sub> sub_tables(const PssmTables &t, size_t m, size_t k)
{
    const bool wide = lds_wide((int)k);
    auto sub = [&](const char *name, size_t off, size_t n) { return Sub{name, off == kAbsent ? nullptr : t.bytes.data() + off, n}; };
    std::vector<Sub> subs = {
        sub("dense", t.dense, m * k * 4),
        sub("table", t.table, k * t.ts * 4),
        sub("table_pad", t.table_pad, k * (size_t)table_stride((int)(m + t.lead), wide) * 4),
        sub("image", t.image, (size_t)prefilter_image_dw((int)m, (int)k) * 4),
        sub("image2", t.image2, (size_t)prefilter2_image_dw((int)m, (int)k) * 4),
        sub("image2_drop", t.image2_drop, (size_t)prefilter2_image_dw((int)m - 1, (int)k) * 4),
        sub("image2_multi", t.image2_multi, (size_t)prefilter2_image_dw((int)m, kDnaMulti) * 4),
    };
    for (size_t i = 0; i < t.parts.size(); ++i)
        subs.push_back(Sub{"part" + std::to_string(i), t.bytes.data() + t.parts[i].table, k * t.parts[i].ts * 4});
    return subs;
}

static void check_layout(const std::string &name, const PssmTables &t, const std::vector<Sub> &subs, size_t m)
{
    std::vector<unsigned char> covered(t.bytes.size(), 0);
    for (const Sub &s : subs) {
        if (!s.p)
            continue;
        const size_t off = (size_t)(s.p - t.bytes.data());
        CHECK(off % 256 == 0, "%s starts at byte %zu, no multiple of 256", s.name.c_str(), off);
        CHECK(s.n > 0 && off <= t.bytes.size() && s.n <= t.bytes.size() - off, "%s [%zu, +%zu) leaves the image of %zu bytes", s.name.c_str(), off,
              s.n, t.bytes.size());
        if (off > t.bytes.size() || s.n > t.bytes.size() - off)
            return;
        for (size_t i = off; i < off + s.n; ++i) {
            CHECK(!covered[i], "%s overlaps another table at byte %zu", s.name.c_str(), i);
            if (covered[i])
                return;
            covered[i] = 1;
        }
    }
    for (size_t i = 0; i < t.bytes.size(); ++i)
        if (!covered[i] && t.bytes[i]) {
            CHECK(false, "padding byte %zu is %u", i, t.bytes[i]);
            break;
        }
    size_t next = 0;
    for (const auto &part : t.parts) {  // slices follow each other; only `lead` rows of a slice are no rows of the motif
        CHECK(part.off == next && part.m > part.lead, "slice at row %zu, expected %zu", part.off, next);
        next = part.off + part.m - part.lead;
    }
    CHECK(t.parts.empty() || next == m, "the slices end at row %zu of %zu", next, m);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <pssm_tables_digest.json>\n", argv[0]);
        return 2;
    }
    // the recorded file: one `"<case>": {...}` per line between the braces
    std::map<std::string, std::string> golden;
    std::ifstream in(argv[1]);
    for (std::string line; std::getline(in, line);) {
        const size_t q0 = line.find('"'), q1 = line.find("\": {");
        if (q0 == std::string::npos || q1 == std::string::npos)
            continue;
        std::string body = line.substr(q1 + 3);
        if (!body.empty() && body.back() == ',')
            body.pop_back();
        golden[line.substr(q0 + 1, q1 - q0 - 1)] = body;
    }
    const std::vector<Case> cases = all_cases();
    for (const Case &c : cases) {
        const std::string &name = c.name;
        const PssmTables t = build_pssm_tables(c.w.data(), c.m, c.k, c.xlong_store);
        const std::vector<Sub> subs = sub_tables(t, c.m, c.k);
        check_layout(name, t, subs, c.m);
        Scalars sc;
        sc.ts = t.ts, sc.lead = t.lead, sc.parts = t.parts, sc.drop_dmax = t.drop_dmax, sc.has_prefilter = t.has_prefilter;
        sc.pre_offset = t.pre_offset, sc.pre_factor = t.pre_factor, sc.pre_emax = t.pre_emax;
        const std::string got = digest(subs, sc);
        const auto want = golden.find(name);
        CHECK(want != golden.end(), "no recorded digest");
        if (want != golden.end())
            CHECK(want->second == got, "digest differs\n  recorded %s\n  built    %s", want->second.c_str(), got.c_str());
    }
    const std::string name = "all";
    CHECK(golden.size() == cases.size(), "%zu recorded digests, %zu cases", golden.size(), cases.size());
    {   // m == 0 stays legal: an empty image
        const PssmTables t = build_pssm_tables(nullptr, 0, 5, true);
        CHECK(t.bytes.empty() && t.dense == kAbsent && t.parts.empty() && !t.has_prefilter, "m = 0 makes %zu bytes", t.bytes.size());
    }
    if (failures) {
        std::fprintf(stderr, "test_pssm_tables: %d checks failed\n", failures);
        return 1;
    }
    std::printf("test_pssm_tables: all checks passed (%zu matrices)\n", cases.size());
    return 0;
}
