// The KXHIPW01 weight container on the host (see kxw_file.h).  Plain C++17, no HIP.
#include "kxw_file.h"

#include <sys/stat.h>
#include <unistd.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace kx {

static_assert(sizeof(size_t) == 8, "container offsets are 64-bit");

template <class U>
static U get(const unsigned char* p) {
    U v;
    memcpy(&v, p, sizeof v);
    return v;
}

KxwHeader kxw_header(const unsigned char* h, size_t have) {
    if (have < KXW_HEADER_BYTES || !is_kxw_magic(h, have)) throw Error(2, "weight blob: bad magic (expected KXHIPW01)");
    KxwHeader r;
    r.n_tensors = get<uint32_t>(h + 8);
    r.total_bytes = get<uint64_t>(h + 24);
    r.table_bytes = KXW_HEADER_BYTES + r.n_tensors * KXW_ENTRY_BYTES;  // (at most 2^39: n_tensors is 32 bits wide)
    if (r.table_bytes > r.total_bytes) throw Error(2, "weight blob: truncated tensor table");
    return r;
}

static std::string shape_str(int ndim, const int* dims) {
    std::string s = "[";
    for (int k = 0; k < ndim; ++k) s += (k ? ", " : "") + std::to_string(dims[k]);
    return s + "]";
}

TensorTable kxw_table(const unsigned char* hdr, size_t hdr_bytes, size_t total_bytes) {
    const KxwHeader h = kxw_header(hdr, hdr_bytes);
    if (h.total_bytes != total_bytes) throw Error(2, "weight blob: size does not match header");
    if (h.table_bytes > hdr_bytes) throw Error(2, "weight blob: truncated tensor table");
    TensorTable table;
    for (size_t i = 0; i < h.n_tensors; ++i) {
        const unsigned char* e = hdr + KXW_HEADER_BYTES + i * KXW_ENTRY_BYTES;
        const size_t name_len = strnlen(reinterpret_cast<const char*>(e), KXW_NAME_BYTES);
        const std::string name(reinterpret_cast<const char*>(e), name_len);
        const uint32_t dt = get<uint32_t>(e + 88), nd = get<uint32_t>(e + 92);
        const uint64_t off = get<uint64_t>(e + 112), nb = get<uint64_t>(e + 120);
        if (name_len == KXW_NAME_BYTES || dt != 0 || nd > 4 || (off % KXW_ALIGN) || off < h.table_bytes || nb > total_bytes ||
            off > total_bytes - nb)
            throw Error(2, "weight blob: bad entry " + name);
        TensorInfo ti;
        ti.offset = off;
        ti.nbytes = nb;
        ti.ndim = (int)nd;
        uint64_t cnt = 1;
        for (uint32_t k = 0; k < nd; ++k) {
            const uint32_t d = get<uint32_t>(e + 96 + 4 * k);
            if (d > (uint32_t)INT_MAX || (d != 0 && cnt > UINT64_MAX / d)) throw Error(2, "weight blob: size mismatch " + name);
            ti.dims[k] = (int)d;
            cnt *= d;
        }
        if (nb % 4 != 0 || cnt != nb / 4) throw Error(2, "weight blob: size mismatch " + name);
        if (!table.emplace(name, ti).second) throw Error(2, "weight blob: bad entry " + name + " (the name appears twice)");
    }
    for (const SpecEntry& s : tensor_spec()) {
        const auto it = table.find(s.name);
        if (it == table.end()) throw Error(2, "weight blob: missing tensor " + s.name);
        const TensorInfo& ti = it->second;
        if (ti.ndim != s.ndim || memcmp(ti.dims, s.dims, sizeof(int) * (size_t)s.ndim) != 0)
            throw Error(2, "weight blob: shape mismatch " + s.name + ": the file has " + shape_str(ti.ndim, ti.dims) + ", the model needs " +
                               shape_str(s.ndim, s.dims));
    }
    return table;
}

std::vector<unsigned char> read_file(const char* path, const char* what) {
    FILE* f = fopen(path, "rb");
    if (!f) throw Error(2, std::string("cannot open ") + what + ": " + path);
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz < 0) {
        fclose(f);
        throw Error(2, std::string("cannot size ") + what + ": " + path);
    }
    std::vector<unsigned char> host((size_t)sz);
    const size_t got = host.empty() ? 0 : fread(host.data(), 1, host.size(), f);
    fclose(f);
    if (got != host.size()) throw Error(2, std::string("short read on ") + what + ": " + path);
    return host;
}

void write_file_atomic(const std::string& path, const void* data, size_t n) {
    const std::string tmp = path + ".tmp." + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) throw Error(2, "cannot write " + path);
    const bool ok = fwrite(data, 1, n, f) == n;
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) {
        (void)remove(tmp.c_str());
        throw Error(2, "short write on " + path);
    }
}

std::vector<unsigned char> import_onnx_bytes(const unsigned char* data, size_t n, int* variant) {
    try {
        ImportInfo info;
        std::vector<unsigned char> blob = onnx_to_kxw(data, n, &info);
        if (variant) *variant = info.variant();
        return blob;
    } catch (const ImportError& e) {
        throw Error(2, std::string("weight file is not a KXHIPW01 blob (bad magic) and not a readable ONNX model: ") + e.what());
    }
}

// The KXHIPW01 image behind `path`.  The path is either the library's own container or — what the reference passes to
// OrtKoko::new (koko.rs:570-573, hf_cache.rs:128-158) — the `.onnx` file, which is converted in memory
// (onnx_import.cpp).
std::vector<unsigned char> read_weight_file(const char* path, int* variant) {
    if (!path || !*path) throw Error(1, "kx_create: empty weights path");
    if (variant) *variant = 0;
    std::vector<unsigned char> host = read_file(path, "weight file");
    if (is_kxw_magic(host.data(), host.size())) {
        if (kxw_header(host.data(), host.size()).total_bytes != host.size()) throw Error(2, "weight blob: file size does not match header");
        return host;
    }
    // The converted image may be cached beside the source -- ONLY when KOKOROX_KXW_CACHE=1 says so (a library should not drop
    // files into a model cache unasked, and a file the library never wrote is never trusted), and only while the cache's stamp
    // names exactly this source: its size, its modification time to the nanosecond and the importer's version (cp -p / mv / a
    // re-pointed Hugging Face blob symlink keep an older mtime: a "not older than the source" test would load the former
    // variant's weights).
    const std::string cache = std::string(path) + ".kxw", stamp_path = cache + ".src";
    const char* ce = getenv("KOKOROX_KXW_CACHE");
    const bool use_cache = ce && strcmp(ce, "1") == 0;
    struct stat so;
    std::string stamp;
    if (use_cache && stat(path, &so) == 0) {
        stamp = "kxw-cache 1 importer " + std::to_string(KX_IMPORTER_VERSION) + " size " + std::to_string((long long)so.st_size) + " mtime " +
                std::to_string((long long)so.st_mtim.tv_sec) + "." + std::to_string((long)so.st_mtim.tv_nsec) + "\n";
        try {
            const std::vector<unsigned char> st = read_file(stamp_path.c_str(), "weight cache stamp");
            if (std::string(st.begin(), st.end()) == stamp) {
                std::vector<unsigned char> c = read_file(cache.c_str(), "weight cache");
                if (kxw_header(c.data(), c.size()).total_bytes == c.size()) {
                    if (variant) *variant = -1;  // (a cached conversion: the source's kind was not looked at again)
                    return c;
                }
            }
        } catch (const Error&) {  // no cache, or an unreadable one, is not an error: convert
        }
    }
    int var = 1;
    std::vector<unsigned char> blob = import_onnx_bytes(host.data(), host.size(), &var);
    if (variant) *variant = var;
    if (var >= 3)
        fprintf(stderr,
                "kokorox-hip: %s is a %d-bit quantised ONNX variant: its weights are de-quantised at load and the model runs f32-class "
                "arithmetic, which is NOT what ONNX Runtime computes for this file (it quantises the activations at run time: "
                "DynamicQuantizeLinear -> MatMulInteger / ConvInteger / MatMulNBits).  Parity with the reference is claimed for "
                "onnx/model.onnx only.\n",
                path, var == 3 ? 8 : 4);
    if (use_cache && !stamp.empty()) {
        try {
            write_file_atomic(cache, blob.data(), blob.size());
            write_file_atomic(stamp_path, stamp.data(), stamp.size());  // (the stamp last: a cache without it is ignored)
        } catch (const Error&) {  // a cache that could not be written is not an error either
        }
    }
    return blob;
}

}  // namespace kx
