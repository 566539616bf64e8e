// sampler_policy_test — every decision of the row / envelope chooser (longtermplanner_amd/csrc/ltp_sampler_policy.hpp) over the
// product of its inputs, on the host, against tests/golden/sampler_policy.txt: the kernel names the dispatch code that the chooser
// replaced reported for the same inputs. Inputs: the flag word (bits 0..7) and every ltp_sample_opts, both semantics, every
// ltp_set_table_pass, stamps on / off, float64 / float32, and caps, strides and joint counts on each side of every threshold.
//   sampler_policy_test FIXTURE      exit status 0 = every decision as recorded
#include "../../longtermplanner_amd/csrc/ltp_sampler_policy.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

using namespace ltp;

static const int kCaps[] = {0, 24, 32, 33, 256, 257, 768, 769, 1024, 1025};
static const int kStrides[] = {1, 2, 3};
// joints on each side of the walk's 2 GiB batch descriptor (sample_walk_applies) at caps of 1024 and 769 samples
static const int kDofs[] = {7, 65535, 65536, 83886, 83887};

static std::vector<std::string> g_names;
static int g_failures = 0;

static int code_of(const char* name)
{
    for (size_t i = 0; i < g_names.size(); ++i)
        if (g_names[i] == name) return (int)i;
    return -1;
}

// the kernel name must name the path it came with
static bool path_matches(const SampleChoice& c)
{
    const std::string n = c.kernel;
    switch (c.path) {
    case SamplePath::Fused: return n == "k_sample" && c.walk_kernel < 0;
    case SamplePath::Table: return n.rfind("k_sample_tab_", 0) == 0 && c.walk_kernel < 0;
    case SamplePath::Walk:
    case SamplePath::WalkAuto:
        return c.walk_kernel >= 0 && c.walk_kernel < kWalkKernelCount && n == kWalkKernelNames[c.walk_kernel] &&
               (n.find("_auto_") != std::string::npos) == (c.path == SamplePath::WalkAuto);
    }
    return false;
}

// run-length form of the fixture: a letter per name code, followed by its repeat count when that is more than 1
static std::vector<int> decode_runs(const std::string& s)
{
    std::vector<int> out;
    for (size_t i = 0; i < s.size();) {
        const char ch = s[i++];
        const int code = ch >= 'A' && ch <= 'Z' ? ch - 'A' : ch >= 'a' && ch <= 'z' ? 26 + ch - 'a' : -1;
        long n = 0;
        while (i < s.size() && s[i] >= '0' && s[i] <= '9') n = 10 * n + (s[i++] - '0');
        out.insert(out.end(), n > 0 ? n : 1, code);
    }
    return out;
}

struct Section {
    std::vector<int> codes;
    size_t next = 0;
    const char* what;
    void check(const char* got, const std::string& input)
    {
        const int want = next < codes.size() ? codes[next] : -1;
        ++next;
        const int have = code_of(got);
        if (have == want && want >= 0) return;
        if (++g_failures <= 20)
            std::printf("MISMATCH %s [%s]: %s, recorded %s\n", what, input.c_str(), got, want >= 0 ? g_names[want].c_str() : "(nothing)");
    }
};

static std::string rows_input(int sem, int tp, int stamps, int f32, int cap, int stride, int dof)
{
    char b[160];
    std::snprintf(b, sizeof b, "semantics %d table_pass %d stamps %d f32 %d cap %d stride %d dof %d", sem, tp, stamps, f32, cap, stride, dof);
    return b;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s FIXTURE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    // "names N" + N lines, then "rows N" / "opts N" / "envelopes N", each followed by run-length lines up to the next section
    Section rows{{}, 0, "flags"}, opts{{}, 0, "opts"}, env{{}, 0, "envelope"};
    Section* cur = nullptr;
    std::string line, runs;
    auto flush = [&]() { if (cur) cur->codes = decode_runs(runs); runs.clear(); };
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        int n = 0;
        char key[32];
        if (line.find(' ') != std::string::npos && std::sscanf(line.c_str(), "%31s %d", key, &n) == 2) {   // (run lines have no blanks)
            flush();
            if (!std::strcmp(key, "names")) {
                for (int i = 0; i < n && std::getline(in, line); ++i) g_names.push_back(line);
                cur = nullptr;
            } else {
                cur = !std::strcmp(key, "rows") ? &rows : !std::strcmp(key, "opts") ? &opts : &env;
                cur->codes.reserve(n);
            }
            continue;
        }
        runs += line;
    }
    flush();

    // the flag word
    long decisions = 0;
    for (int flags = 0; flags < 256; ++flags) {
        const SamplePolicy pol = policy_from_flags(flags | (37 << 8));
        if (pol.interleave != 37) { std::printf("MISMATCH flags %d: interleave %d\n", flags, pol.interleave); ++g_failures; }
        for (int sem = 0; sem < 2; ++sem)
            for (int tp = -1; tp <= 1; ++tp)
                for (int stamps = 0; stamps < 2; ++stamps)
                    for (int f32 = 0; f32 < 2; ++f32)
                        for (int cap : kCaps)
                            for (int stride : kStrides)
                                for (int dof : kDofs) {
                                    const SampleChoice c = choose_sampler(pol, sem, tp, stamps, f32, RowSpec{cap, stride}, dof);
                                    const std::string what = "flags " + std::to_string(flags) + " " + rows_input(sem, tp, stamps, f32, cap, stride, dof);
                                    if (!path_matches(c)) { std::printf("MISMATCH path of %s [%s]\n", c.kernel, what.c_str()); ++g_failures; }
                                    rows.check(c.kernel, what);
                                    ++decisions;
                                }
    }
    // ltp_sample_opts (the element type is the format's)
    for (int stores = 0; stores < 2; ++stores)
        for (int sampler = LTP_SAMPLER_AUTO; sampler <= LTP_SAMPLER_TABLE; ++sampler)
            for (int verdict = 0; verdict < 2; ++verdict)
                for (int dry = 0; dry < 2; ++dry)
                    for (int format = 0; format < 2; ++format) {
                        ltp_sample_opts o{sizeof(ltp_sample_opts), format, stores, sampler, verdict, 4242, dry};
                        const SamplePolicy pol = policy_from_opts(o);
                        if (pol.interleave != 4242) { std::printf("MISMATCH opts: interleave %d\n", pol.interleave); ++g_failures; }
                        for (int sem = 0; sem < 2; ++sem)
                            for (int tp = -1; tp <= 1; ++tp)
                                for (int stamps = 0; stamps < 2; ++stamps)
                                    for (int cap : kCaps)
                                        for (int stride : kStrides)
                                            for (int dof : kDofs) {
                                                const SampleChoice c = choose_sampler(pol, sem, tp, stamps, format == LTP_ROWS_F32, RowSpec{cap, stride}, dof);
                                                char b[96];
                                                std::snprintf(b, sizeof b, "stores %d sampler %d verdict %d dry %d format %d ", stores, sampler, verdict, dry, format);
                                                const std::string what = b + rows_input(sem, tp, stamps, format, cap, stride, dof);
                                                if (!path_matches(c)) { std::printf("MISMATCH path of %s [%s]\n", c.kernel, what.c_str()); ++g_failures; }
                                                opts.check(c.kernel, what);
                                                ++decisions;
                                            }
                    }
    // envelopes
    for (int mode = 0; mode < 2; ++mode)
        for (int sem = 0; sem < 2; ++sem)
            for (int tp = -1; tp <= 1; ++tp)
                for (int stamps = 0; stamps < 2; ++stamps) {
                    const EnvelopeChoice c = choose_envelope(mode, sem, tp, stamps);
                    char b[96];
                    std::snprintf(b, sizeof b, "mode %d semantics %d table_pass %d stamps %d", mode, sem, tp, stamps);
                    if (c.path != EnvelopePath::Walk && c.analytic != (mode == LTP_ENVELOPE_ANALYTIC)) {
                        std::printf("MISMATCH envelope form [%s]\n", b);
                        ++g_failures;
                    }
                    env.check(c.kernel, b);
                    ++decisions;
                }
    for (Section* s : {&rows, &opts, &env})
        if (s->next != s->codes.size()) {
            std::printf("MISMATCH %s: %zu decisions, %zu recorded\n", s->what, s->next, s->codes.size());
            ++g_failures;
        }
    std::printf("%ld decisions, %d mismatches\n", decisions, g_failures);
    return g_failures ? 1 : 0;
}
