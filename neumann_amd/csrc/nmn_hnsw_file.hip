// nmn_hnsw_file.hip — the HNSW index file (docs/hnsw.md §10): save, load, and the config a loaded handle reports.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device:
// every distance restates the reference's unfused f32 arithmetic and must give its bits (docs/hnsw.md, "Source layout").
// (A load recomputes every row's magnitude with the host arithmetic of nmn_hnsw_arith.h and compares its bits with the file's.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <shared_mutex>
#include <string>
#include <vector>

#include "nmn_hnsw_handle.h"

#pragma clang fp contract(off)

using namespace nmn;
using namespace nmn::hnsw;

// ---- persistence (docs/hnsw.md §10) ----------------------------------------------------------------------------------------------
// File = PersistHeader{kind = hnsw, flags bit 0 = quantized, rows = n, aux = graph bytes, reserved = FNV-1a 64 of the graph section}
// | graph section (config, rng, entry, max_layer, n_upper, levels, layer-0 counts, layer-0 ids, upper lists) | rows section.
// No kernel of its own: a load is sequential reads, host checks and bulk copies.  Nothing of a file reaches hnsw_search_kernel
// before the host has proved every id of it in bounds (a neighbour id >= n, or a level-0 node listed on an upper layer, whose up_idx
// is kNone, would be an out-of-bounds read on the device).
#include "nmn_persist.h"

static_assert(sizeof(nmn_hnsw_config) == 48, "nmn_hnsw_config is part of the file format");

static const char* const kSaveSparseRefusal =
    "HNSW: the index holds sparse nodes (nmn_hnsw_insert_sparse / nmn_hnsw_insert_auto) and index file format version 1 has no place "
    "for their stored entries; saving it would lose them";
static const char* const kSaveTTRefusal =
    "HNSW: the index holds TensorTrain nodes (nmn_hnsw_insert_embedding_tt) and index file format version 1 has no place for their "
    "trains and cached norms; saving it would lose them";

namespace {

constexpr uint64_t kGraphFixed = 48 + 8 + 8 + 4 + 4;  // config, rng, entry_point, max_layer, n_upper

uint64_t fnv1a64(const uint8_t* p, size_t n) {
    uint64_t hsh = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) hsh = (hsh ^ p[i]) * 0x100000001b3ull;
    return hsh;
}

template <typename T>
void put(std::vector<uint8_t>& b, const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}

nmn_status bad_file(const std::string& what) { return set_error(NMN_ERR_SERIALIZATION, ("HNSW index file: " + what).c_str()); }

// a cursor over the graph section: every read is checked against the section's end
struct Cursor {
    const uint8_t* p;
    uint64_t left;
    template <typename T>
    bool get(T* out) {
        if (left < sizeof(T)) return false;
        memcpy(out, p, sizeof(T));
        p += sizeof(T);
        left -= sizeof(T);
        return true;
    }
};

// one neighbour list: count <= cap, ids < n, strictly ascending, every id of level >= layer
nmn_status read_list(Cursor& c, uint32_t count, uint32_t n, uint32_t layer, const std::vector<uint8_t>& level, uint32_t node,
                     std::vector<uint32_t>* out) {
    if ((uint64_t)count * 4 > c.left) return bad_file("graph section truncated (neighbour ids)");
    out->resize(count);
    if (count) memcpy(out->data(), c.p, (size_t)count * 4);
    c.p += (size_t)count * 4;
    c.left -= (uint64_t)count * 4;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t id = (*out)[i];
        const std::string at = " (node " + std::to_string(node) + ", layer " + std::to_string(layer) + ")";
        if (id >= n) return bad_file("neighbour id " + std::to_string(id) + " out of range" + at);
        if (i && id <= (*out)[i - 1]) return bad_file("neighbour list not strictly ascending" + at);
        if (level[id] < layer) return bad_file("neighbour id " + std::to_string(id) + " does not reach the layer it is listed on" + at);
    }
    return NMN_OK;
}

}  // namespace

namespace nmn {

nmn_status persist_write_hnsw(nmn_hnsw* h, FILE* fp, const char* path) {
    std::shared_lock<std::shared_mutex> g(h->rw);  // searches may run, inserts wait
    if (h->n_sparse) return set_error(NMN_ERR_CONFIGURATION, kSaveSparseRefusal);
    if (!h->tt_nodes.empty()) return set_error(NMN_ERR_CONFIGURATION, kSaveTTRefusal);
    const uint64_t n = h->level.size();
    const uint32_t dim = h->dim;
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED;
    std::vector<uint8_t> sec;
    nmn_hnsw_config cfg = h->cfg;
    cfg.storage = h->storage;
    cfg.reserved = 0;
    put(sec, cfg);
    put(sec, h->rng);
    put(sec, n ? h->entry : ~0ull);
    put(sec, h->max_layer);
    uint32_t n_upper = 0;
    for (uint8_t l : h->level) n_upper += l > 0 ? 1u : 0u;
    put(sec, n_upper);
    sec.insert(sec.end(), h->level.begin(), h->level.end());
    sec.resize((sec.size() + 3) & ~(size_t)3, 0);
    for (uint64_t i = 0; i < n; i++) put(sec, (uint32_t)h->nbr[i][0].size());
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t id : h->nbr[i][0]) put(sec, id);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t l = 1; l <= h->level[i]; l++) {
            put(sec, (uint32_t)h->nbr[i][l].size());
            for (uint32_t id : h->nbr[i][l]) put(sec, id);
        }
    PersistHeader hd{};
    memcpy(hd.magic, "NMNIDX\0\1", 8);
    hd.version = 1;
    hd.kind = kPersistHnsw;
    hd.dim = dim;
    hd.flags = q8 ? 1u : 0u;
    hd.rows = n;
    hd.row_base = 0;
    hd.aux = sec.size();
    hd.reserved = fnv1a64(sec.data(), sec.size());
    uint64_t rows_bytes = 0;
    if (n) rows_bytes = q8 ? n * dim + n * 16ull : sizeof(PersistHeader) + n * dim * 4ull + n * 4ull;
    hd.payload_bytes = hd.aux + rows_bytes;
    if (fwrite(&hd, sizeof hd, 1, fp) != 1 || fwrite(sec.data(), 1, sec.size(), fp) != sec.size())
        return persist_io_error("cannot write", path);
    if (n == 0) return NMN_OK;
    if (!q8)  // the handle's flat index, from the host's copy of it: the same rows, the same magnitudes, no device traffic
        return persist_write_rows_host(fp, path, dim, n, 0, h->rows.data(), h->mags.data());
    std::vector<float> rec((size_t)n * 4);
    for (uint64_t i = 0; i < n; i++) {
        rec[4 * i + 0] = h->qscale[i];
        rec[4 * i + 1] = h->qmin[i];
        rec[4 * i + 2] = h->mags[i];
        rec[4 * i + 3] = h->qxsq[i];
    }
    if (fwrite(h->codes.data(), dim, n, fp) != n || fwrite(rec.data(), 16, n, fp) != n) return persist_io_error("cannot write", path);
    return NMN_OK;
}

// the file persist_write_hnsw wrote, header already read into hd (persist_read_header: magic, version, payload within the file)
nmn_status persist_read_hnsw(FILE* fp, const char* path, const PersistHeader& hd, int32_t device, uint64_t capacity_hint,
                             nmn_hnsw** out) {
    *out = nullptr;
    if (hd.kind != kPersistHnsw) return bad_file("not an HNSW index file (another kind of section)");
    if (hd.dim == 0 || hd.dim > kMaxDim) return bad_file("dimension out of range (1 .. 8192)");
    if (hd.flags & ~1u) return bad_file("unknown flag bits");
    if (hd.row_base != 0) return bad_file("row_base must be 0");
    const bool q8 = (hd.flags & 1u) != 0;
    const uint32_t dim = hd.dim;
    // sizes: everything announced must be in the file before it sizes anything
    const uint64_t left = persist_bytes_left(fp);
    if (left == UINT64_MAX) return set_error(NMN_ERR_IO, "IO error: cannot seek in the index file");
    if (hd.payload_bytes != left) return bad_file("payload_bytes differs from the bytes that follow the header");
    if (hd.aux > hd.payload_bytes || hd.aux < kGraphFixed) return bad_file("graph section size is inconsistent with the file");
    if (hd.rows > hd.aux / 4 || hd.rows >= (uint64_t)kNone) return bad_file("node count is inconsistent with the graph section size");
    const uint64_t n64 = hd.rows;
    const uint32_t n = (uint32_t)n64;
    {
        unsigned __int128 rows_bytes = 0;
        if (n64) rows_bytes = q8 ? (unsigned __int128)n64 * dim + (unsigned __int128)n64 * 16
                                 : (unsigned __int128)sizeof(PersistHeader) + (unsigned __int128)n64 * dim * 4 + (unsigned __int128)n64 * 4;
        if ((unsigned __int128)hd.aux + rows_bytes != (unsigned __int128)hd.payload_bytes)
            return bad_file("payload_bytes is inconsistent with the node count and the dimension");
    }
    std::vector<uint8_t> sec((size_t)hd.aux);
    if (fread(sec.data(), 1, sec.size(), fp) != sec.size()) return bad_file("truncated (graph section)");
    if (fnv1a64(sec.data(), sec.size()) != hd.reserved) return bad_file("corrupt: graph section checksum mismatch");
    Cursor c{sec.data(), hd.aux};
    nmn_hnsw_config cfg;
    uint64_t rng = 0, entry = 0;
    uint32_t max_layer = 0, n_upper = 0;
    (void)c.get(&cfg);  // (aux >= kGraphFixed)
    (void)c.get(&rng);
    (void)c.get(&entry);
    (void)c.get(&max_layer);
    (void)c.get(&n_upper);
    if (cfg.storage == NMN_HNSW_STORAGE_AUTO) return bad_file("config storage is Auto, which no handle has");
    if (cfg.storage != (q8 ? NMN_HNSW_STORAGE_QUANTIZED : NMN_HNSW_STORAGE_DENSE)) return bad_file("config storage differs from the header's flag");
    if (cfg.reserved != 0) return bad_file("config reserved field is not 0");
    nmn_hnsw_config cfg_dense = cfg;
    cfg_dense.storage = NMN_HNSW_STORAGE_DENSE;  // (check_cfg and create_handle take the strategy apart from the config)
    if (check_cfg(&cfg_dense) != NMN_OK) return bad_file(std::string("invalid config: ") + nmn_last_error());
    if (cfg.max_nodes > 0 && n64 > cfg.max_nodes) return bad_file("more nodes than the config's max_nodes");
    if (rng == 0) return bad_file("rng state is 0 (the xorshift generator never reaches it)");
    if (n == 0) {
        if (entry != ~0ull || max_layer != 0 || n_upper != 0) return bad_file("an empty index with an entry point, a layer or upper nodes");
    } else if (entry >= n64) {
        return bad_file("entry point out of range");
    }
    // levels, zero-padded to 4 bytes
    const uint64_t lv_bytes = ((uint64_t)n + 3) & ~3ull;
    if (lv_bytes > c.left) return bad_file("graph section truncated (levels)");
    std::vector<uint8_t> level(c.p, c.p + n);
    for (uint64_t i = n; i < lv_bytes; i++)
        if (c.p[i] != 0) return bad_file("level padding is not zero");
    c.p += lv_bytes;
    c.left -= lv_bytes;
    uint32_t top = 0, upper = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (level[i] > 32) return bad_file("level of node " + std::to_string(i) + " above 32");
        top = std::max<uint32_t>(top, level[i]);
        upper += level[i] > 0 ? 1u : 0u;
    }
    if (n) {
        if (max_layer != top) return bad_file("max_layer differs from the highest level");
        if (level[entry] != max_layer) return bad_file("the entry point's level is not max_layer");
        if (n_upper != upper) return bad_file("n_upper differs from the count of nodes of level >= 1");
    }
    // layer 0: counts, then the lists
    if ((uint64_t)n * 4 > c.left) return bad_file("graph section truncated (layer-0 counts)");
    std::vector<uint32_t> l0cnt(n);
    if (n) memcpy(l0cnt.data(), c.p, (size_t)n * 4);
    c.p += (size_t)n * 4;
    c.left -= (uint64_t)n * 4;
    for (uint32_t i = 0; i < n; i++)
        if (l0cnt[i] > cfg.m0) return bad_file("layer-0 count of node " + std::to_string(i) + " above m0");
    std::vector<std::vector<std::vector<uint32_t>>> nbr(n);
    nmn_status st = NMN_OK;
    for (uint32_t i = 0; i < n; i++) {
        nbr[i].resize((size_t)level[i] + 1);
        st = read_list(c, l0cnt[i], n, 0, level, i, &nbr[i][0]);
        if (st != NMN_OK) return st;
    }
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t l = 1; l <= level[i]; l++) {
            uint32_t cnt = 0;
            if (!c.get(&cnt)) return bad_file("graph section truncated (upper-layer count)");
            if (cnt > cfg.m) return bad_file("upper-layer count of node " + std::to_string(i) + " above m");
            st = read_list(c, cnt, n, l, level, i, &nbr[i][l]);
            if (st != NMN_OK) return st;
        }
    if (c.left != 0) return bad_file("trailing bytes in the graph section");
    sec.clear();
    sec.shrink_to_fit();

    // rows: read and proved on the host
    std::vector<float> rows, mags, qscale, qmin, qxsq;
    std::vector<uint8_t> codes;
    if (n && !q8) {
        PersistHeader hv{};
        st = persist_read_header(fp, path, &hv);
        if (st != NMN_OK) return st;
        if (hv.kind != kPersistFlat || hv.dim != dim || hv.rows != n64 || hv.row_base != 0 ||
            hv.payload_bytes != n64 * dim * 4ull + n64 * 4ull)
            return bad_file("the rows section's header is inconsistent with the index");
        st = persist_read_rows_host(fp, hv, &rows, &mags);  // (its checksum)
        if (st != NMN_OK) return st;
        for (uint32_t i = 0; i < n; i++) {
            const float* v = rows.data() + (size_t)i * dim;
            const float m = sqrtf(h_dot8(v, v, dim));
            if (memcmp(&m, &mags[i], 4) != 0) return bad_file("corrupt: row magnitudes differ from the stored ones (row " + std::to_string(i) + ")");
        }
    } else if (n) {
        codes.resize((size_t)n * dim);
        std::vector<float> rec((size_t)n * 4);
        if (fread(codes.data(), dim, n, fp) != n || fread(rec.data(), 16, n, fp) != n) return bad_file("truncated (quantized rows)");
        rows.resize((size_t)n * dim);
        mags.resize(n);
        qscale.resize(n);
        qmin.resize(n);
        qxsq.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            qscale[i] = rec[4 * (size_t)i + 0];
            qmin[i] = rec[4 * (size_t)i + 1];
            const uint8_t* code = codes.data() + (size_t)i * dim;
            float* v = rows.data() + (size_t)i * dim;
            h_dequantize(code, dim, qscale[i], qmin[i], v);
            mags[i] = sqrtf(h_dot8(v, v, dim));
            qxsq[i] = h_q8_sqmag(code, qscale[i], qmin[i], dim);
            if (memcmp(&mags[i], &rec[4 * (size_t)i + 2], 4) != 0 || memcmp(&qxsq[i], &rec[4 * (size_t)i + 3], 4) != 0)
                return bad_file("corrupt: quantized row " + std::to_string(i) + " does not give its stored magnitude / squared magnitude");
        }
    }
    if (persist_bytes_left(fp) != 0) return bad_file("trailing bytes after the rows section");

    // the handle: device arrays sized by numbers the checks above have bounded by the file's size
    nmn_hnsw* h = nullptr;
    st = create_handle(&cfg_dense, q8 ? NMN_HNSW_STORAGE_QUANTIZED : NMN_HNSW_STORAGE_DENSE, dim, std::max<uint64_t>(capacity_hint, n64),
                       device, &h);
    if (st != NMN_OK) return st;
    auto fail_with = [&](nmn_status s) {
        const std::string keep = nmn_last_error();
        nmn_hnsw_destroy(h);
        return set_error(s, keep.c_str());
    };
    h->rows = std::move(rows);
    h->mags = std::move(mags);
    h->codes = std::move(codes);
    h->qscale = std::move(qscale);
    h->qmin = std::move(qmin);
    h->qxsq = std::move(qxsq);
    h->level = std::move(level);
    h->nbr = std::move(nbr);
    h->entry = n ? entry : ~0ull;
    h->max_layer = max_layer;
    h->rng = rng;
    if (n && !q8) {
        st = nmn_index_upload(h->vectors, h->rows.data(), 0, n64);  // H2D + the magnitudes in reference order, on the device
        if (st != NMN_OK) return fail_with(st);
        std::vector<float> got(n);
        const hipError_t e = hipMemcpy(got.data(), h->vectors->norms, (size_t)n * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail_with(set_error_hip(e, "reading the magnitudes back"));
        if (memcmp(got.data(), h->mags.data(), (size_t)n * 4) != 0)
            return fail_with(bad_file("corrupt: the device's row magnitudes differ from the stored ones"));
    } else if (n) {
        st = upload_codes(h, 0, n64);
        if (st != NMN_OK) return fail_with(st);
    }
    st = upload_graph(h);
    if (st != NMN_OK) return fail_with(st);
    *out = h;
    return NMN_OK;
}

}  // namespace nmn

extern "C" nmn_status nmn_hnsw_get_config(const nmn_hnsw* h, nmn_hnsw_config* out) {
    if (!h || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = h->cfg;
    out->storage = h->storage;
    out->reserved = 0;
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_save(nmn_hnsw* h, const char* path) {
    if (!h || !path) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_save", "the file format has no Binary rows section yet"); sb != NMN_OK) return sb;
    {
        std::shared_lock<std::shared_mutex> g(h->rw);
        if (h->n_sparse) return set_error(NMN_ERR_CONFIGURATION, kSaveSparseRefusal);  // before the file is touched
        if (!h->tt_nodes.empty()) return set_error(NMN_ERR_CONFIGURATION, kSaveTTRefusal);
    }
    FILE* fp = fopen(path, "wb");
    if (!fp) return persist_io_error("cannot create", path);
    nmn_status st = persist_write_hnsw(h, fp, path);
    if (fclose(fp) != 0 && st == NMN_OK) st = persist_io_error("cannot close", path);
    return st;
}

extern "C" nmn_status nmn_hnsw_load(const char* path, int32_t device, uint64_t capacity_hint, uint64_t max_file_bytes,
                                    uint64_t max_entries, nmn_hnsw** out) {
    if (!path || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_status st = persist_check_file_size(path, max_file_bytes, nullptr);
    if (st != NMN_OK) return st;
    FILE* fp = fopen(path, "rb");
    if (!fp) return persist_io_error("cannot open", path);
    PersistHeader hd{};
    st = persist_read_header(fp, path, &hd);
    if (st == NMN_OK) st = persist_check_entries(hd.rows, max_entries);
    if (st == NMN_OK) st = persist_read_hnsw(fp, path, hd, device, capacity_hint, out);
    fclose(fp);
    return st;
}
