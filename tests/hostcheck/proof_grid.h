// tests/hostcheck/proof_grid.h — TEST-ONLY: the fixed grid of proof planner inputs behind tests/golden/proof_plans.txt and the line format of that
// file.  proof_plancheck.cpp walks it over csrc/proof_plan.h; the golden file was recorded by walking the same grid over the text of proof_enqueue as
// it stood inside poly.hip before the planner became a header, its launches, copies, reserves and stream calls replaced by calls of these print
// functions (profiles/scalar_drivers.md).  Nothing here knows a plan's layout.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_fr.h"

constexpr int PROOF_GRID_CASES = 29 * 2 * 2 * 3 * 3;
enum ProofGridZ { PGZ_OFF, PGZ_KNOWN, PGZ_ON };         // z off the domain; z = w^(n-1) and the index search finds n - 1; z = w^(n-1) and it finds nothing
enum ProofGridSrc { PGS_HOST, PGS_SET, PGS_RESIDENT };  // evaluations: a host pointer; already in set.a; in a device buffer of the caller's
static const char* const PROOF_GRID_Z[3] = {"off", "known", "on"};
static const char* const PROOF_GRID_SRC[3] = {"host", "set", "resident"};

// f(log_n, want_proof, skip_intt, z kind, source)
template <class F> void proof_grid(F&& f) {
    for (int log_n = 0; log_n <= 28; ++log_n)
        for (int want = 1; want >= 0; --want)
            for (int skip = 0; skip < 2; ++skip)
                for (int zk = 0; zk < 3; ++zk)
                    for (int src = 0; src < 3; ++src) f(log_n, want != 0, skip != 0, (ProofGridZ)zk, (ProofGridSrc)src);
}
// the point of a case (wire): 7, which lies on no domain, or w_n^(n-1) = w_n^-1
inline void proof_grid_z(ProofGridZ kind, int log_n, uint64_t z[4]) {
    const uint64_t seven[4] = {7, 0, 0, 0};
    if (kind == PGZ_OFF) kzg_host::fr_mul(kzg_host::FR_R2, seven, z);
    else memcpy(z, kzg_host::fr_roots().winv[log_n], 32);
}

// The file is written without repetition.  What depends on the size alone is a `size` line (workgroups of the per-element kernels, bytes reserved in
// set.b / .c / .small), printed when it changes.  A plan is two parts, each written once and then named by its number: the chain `C<i>` (form, whether the
// auxiliary stream was asked for, then every step up to the read-back of y) and the tail `T<i>` (the twiddle tables fetched -- f: forward, fi: and
// inverse -- then every step behind the read-back; in the table form, which has no read-back, every step).  One `proof` line per (log_n, want, skip)
// names the plan of its nine cases as `C<i>+T<j>`, three per place of z (off / known / on) in the order host, set, resident; the reserve of set.a is the reserve of set.c unless `,a=<bytes>` says otherwise.
struct ProofTable {
    std::vector<std::string> chains, tails;     // the parts printed so far
    std::string chain, tail;                    // the case being printed
    bool in_tail = false;
    std::string head_chain, head_tail, size, size_printed, label, group_key, group, defs;
    size_t a = 0, c = 0;
};
inline ProofTable& proof_table() { static ProofTable t; return t; }
inline void proof_line(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline void proof_line(const char* fmt, ...) {      // one step of the case being printed
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ProofTable& t = proof_table();
    (t.in_tail ? t.tail : t.chain) += std::string("; ") + buf;
}
inline void proof_flush_group() {
    ProofTable& t = proof_table();
    if (!t.group.empty()) printf("%s%s ->%s\n", t.defs.c_str(), t.group_key.c_str(), t.group.c_str());
    t.group.clear(); t.defs.clear();
}

inline void proof_print_case(int log_n, bool want, bool skip, ProofGridZ zk, ProofGridSrc src) {
    ProofTable& t = proof_table();
    char buf[96];
    snprintf(buf, sizeof buf, "proof log_n=%d want=%d skip=%d", log_n, (int)want, (int)skip);
    if (t.group_key != buf) { proof_flush_group(); t.group_key = buf; }
    t.label = src == PGS_HOST ? std::string(PROOF_GRID_Z[zk]) + ": " : "";      // the sources follow in the grid's order: host, set, resident
}
// the plan's head: form (table / small / levels), workgroups of the per-element kernels, the bytes reserved in set.a (0: no reserve) .b .c .small,
// whether the inverse twiddle tables were fetched beside the forward ones, whether the auxiliary stream was asked for
inline void proof_print_plan(const char* form, uint32_t blocks, size_t a, size_t b, size_t c, size_t small, bool inv_tables, bool aux) {
    ProofTable& t = proof_table();
    char buf[160];
    snprintf(buf, sizeof buf, "size blocks=%u b=%zu c=%zu small=%zu\n", blocks, b, c, small);
    t.size = buf;
    t.a = a; t.c = c;
    t.head_chain = std::string("form=") + form + (aux ? " aux=1" : " aux=0");
    t.head_tail = inv_tables ? "tables=fi" : "tables=f";
}
// a location inside set.b: the n inverses at its head, or a word offset inside the level scratch behind them
inline std::string proof_loc(bool inv, size_t off) { return inv ? std::string("inv") : "lvl+" + std::to_string(off); }
inline const char* proof_stream(bool aux) { return aux ? "aux" : "main"; }
// the once-per-size build of the known-index table: bytes of the z = 1 scalars, bytes of the table, the one-workgroup kernel's LDS and domain
inline void proof_print_build(size_t z1_bytes, size_t table_bytes, size_t lds, int log_ns) { proof_line("build z1=%zu table=%zu lds=%zu log_ns=%d", z1_bytes, table_bytes, lds, log_ns); }
inline void proof_print_upload_scalars(bool aux, size_t bytes) { proof_line("upload_scalars %s bytes=%zu", proof_stream(aux), bytes); }
inline void proof_print_upload_evals(bool aux, size_t bytes) { proof_line("upload_evals %s bytes=%zu", proof_stream(aux), bytes); }
inline void proof_print_inv_small(bool aux, size_t lds, int log_ns, bool out_inv, size_t out_off) {
    proof_line("k_poly_inv_small %s lds=%zu log_ns=%d out=%s", proof_stream(aux), lds, log_ns, proof_loc(out_inv, out_off).c_str());
}
inline void proof_print_inv_level(bool aux, uint32_t grid, int log_l, size_t next_off, size_t out_off) {
    proof_line("k_poly_inv_level %s grid=%u log_l=%d next=%s out=%s", proof_stream(aux), grid, log_l, proof_loc(false, next_off).c_str(), proof_loc(false, out_off).c_str());
}
inline void proof_print_check() { proof_line("check"); }                    // hipGetLastError
inline void proof_print_record(bool aux) { proof_line("record %s", proof_stream(aux)); }
inline void proof_print_join(bool aux) { proof_line("join %s", proof_stream(aux)); }          // the stream that waits
inline void proof_print_inverses(bool aux, uint32_t grid, bool next_inv, size_t next_off, int direct, int fused_y) {
    proof_line("k_poly_inverses %s grid=%u next=%s direct=%d fused_y=%d", proof_stream(aux), grid, proof_loc(next_inv, next_off).c_str(), direct, fused_y);
}
inline void proof_print_kernel(const char* name, bool aux, uint32_t grid) { proof_line("%s %s grid=%u", name, proof_stream(aux), grid); }
inline void proof_print_read_y(bool aux, size_t bytes) { proof_line("read_y %s bytes=%zu", proof_stream(aux), bytes); proof_table().in_tail = true; }
inline void proof_print_intt(bool aux) { proof_line("intt %s", proof_stream(aux)); }
inline size_t proof_part_id(std::vector<std::string>& seen, const std::string& part, char letter, std::string& defs) {
    size_t id = 0;
    while (id < seen.size() && seen[id] != part) ++id;
    if (id == seen.size()) { seen.push_back(part); defs += letter + std::to_string(id) + " " + part + "\n"; }
    return id;
}
// after the last step of a case
inline void proof_end_case() {
    ProofTable& t = proof_table();
    if (!t.in_tail) { t.tail = t.chain; t.chain.clear(); }          // no read-back: the table form
    if (t.size != t.size_printed) { t.defs += t.size; t.size_printed = t.size; }
    const size_t ci = proof_part_id(t.chains, t.head_chain + t.chain, 'C', t.defs), ti = proof_part_id(t.tails, t.head_tail + t.tail, 'T', t.defs);
    t.group += " " + t.label + "C" + std::to_string(ci) + "+T" + std::to_string(ti);
    if (t.a != t.c) t.group += ",a=" + std::to_string(t.a);
    t.chain.clear(); t.tail.clear(); t.in_tail = false;
}
// after the last case
inline void proof_end_table() { proof_flush_group(); }
