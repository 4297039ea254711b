// sum_plan_check.cpp -- Gradient.sum's batch planner (sketchml_amd/csrc/skml_sparse_sum_plan.hpp,
// plan_sum_batches) against the plans tests/test_sum_plan_cpu.py works out in Python's unbounded
// integers.  A stand-alone program: built with g++ by that test (with -fsanitize=address,undefined),
// it reads the script the test writes and prints "ok <checks> checks".
//
//   sum_plan_check <script>
//
// One plan a line, numbers in decimal (needs and budget up to SIZE_MAX):
//   plan budget P need* nb end*        the P needs, then the expected batch ends
// Besides the expected ends, every plan is held to the planner's contract: the ends ascend strictly
// and finish at P (every payload in exactly one batch, in order), and a batch of more than one
// payload sums to at most the budget (the sum taken in 128 bits).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../sketchml_amd/csrc/skml_sparse_sum_plan.hpp"

namespace {

int g_line = 0, g_checks = 0;

[[noreturn]] void die(const std::string& what) {
    std::printf("line %d: %s\n", g_line, what.c_str());
    std::exit(1);
}
void expect(bool ok, const char* what) {
    g_checks++;
    if (!ok) die(what);
}

struct Tokens {
    std::istringstream in;
    explicit Tokens(const std::string& s) : in(s) {}
    std::string word() {
        std::string t;
        if (!(in >> t)) die("the script line ends early");
        return t;
    }
    size_t num() { return (size_t)std::strtoull(word().c_str(), nullptr, 10); }
};

void check_plan(Tokens& tk) {
    static_assert(sizeof(size_t) == 8, "the script's numbers are 64-bit");
    const size_t budget = tk.num();
    std::vector<size_t> need(tk.num());
    for (auto& n : need) n = tk.num();
    std::vector<size_t> want(tk.num());
    for (auto& e : want) e = tk.num();
    const std::vector<size_t> ends = skml::plan_sum_batches(need, budget);
    expect(ends.size() == want.size(), "the number of batches");
    for (size_t b = 0; b < ends.size(); b++) expect(ends[b] == want[b], "a batch end");
    expect(need.empty() ? ends.empty() : (!ends.empty() && ends.back() == need.size()), "the last batch ends at P");
    size_t at = 0;
    for (const size_t end : ends) {
        expect(end > at && end <= need.size(), "a batch takes at least one payload, in order");
        unsigned __int128 bytes = 0;
        for (size_t p = at; p < end; p++) bytes += need[p];
        expect(end - at == 1 || bytes <= budget, "a batch of several payloads fits the budget");
        // greedy: the next payload did not fit
        if (end < need.size()) expect(bytes + need[end] > budget, "a batch stops only at a payload that does not fit");
        at = end;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: sum_plan_check <script>\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    if (!f) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(f, line)) {
        g_line++;
        if (line.empty()) continue;
        Tokens tk(line);
        const std::string cmd = tk.word();
        if (cmd == "plan")
            check_plan(tk);
        else
            die("unknown command " + cmd);
    }
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
