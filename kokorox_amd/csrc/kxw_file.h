// The KXHIPW01 weight container on the host: the one reader of weight files, the one place a tensor table is accepted, and
// the opt-in cache of converted `.onnx` files.  Plain C++17, no HIP: Model keeps only the device side (model.hip:
// load_file, load_device_blob), and the CPU suite builds this unit with g++ -fsanitize=address,undefined (tests/cpp/kxw_fuzz.cpp).
//
// Layout (little endian; written by kokorox_amd/weights.py and onnx_import.cpp):
//     0   char[8] magic "KXHIPW01"      8  u32 n_tensors      12  u32 n_tensors * 128
//     16  u64 data_offset               24 u64 total_bytes    32..63 reserved
//     64  n_tensors entries of 128 bytes: char name[88]; u32 dtype (0 = f32); u32 ndim; u32 dims[4]; u64 offset; u64 nbytes
#pragma once
#include <cstddef>
#include <map>
#include <string>
#include <vector>

#include "kx_error.h"
#include "onnx_import.h"

namespace kx {

constexpr size_t KXW_HEADER_BYTES = 64, KXW_ENTRY_BYTES = 128, KXW_NAME_BYTES = 88, KXW_ALIGN = 256;

struct TensorInfo {
    size_t offset = 0, nbytes = 0;
    int ndim = 0;
    int dims[4] = {0, 0, 0, 0};
};
using TensorTable = std::map<std::string, TensorInfo>;

struct KxwHeader {
    size_t total_bytes, n_tensors;
    size_t table_bytes;  // header + table = 64 + n_tensors * 128: what kxw_table reads, and where tensor data may begin
};
// The first 64 bytes of a container.  Error(KX_ERR_IO): fewer than 64 bytes, wrong magic, a table that does not fit into
// total_bytes.
KxwHeader kxw_header(const unsigned char* h, size_t have);

// Header and table of a container of `total_bytes` -> its tensors.  Every entry must be f32 with at most 4 dimensions, lie
// 256-aligned behind the table and inside the container, hold exactly the bytes of its shape, and have a name of its own;
// and every tensor of tensor_spec() must be there with the spec's shape, because Model::build and the forward hard-code the
// architecture: a smaller tensor would be read past its end on the GPU.  Entries the spec does not know are ignored (Model
// never reads them).  Error(KX_ERR_IO) otherwise; nothing of the tensor data is needed.
TensorTable kxw_table(const unsigned char* hdr, size_t hdr_bytes, size_t total_bytes);

// `what` names the file's role in the messages: "cannot open <what>: <path>", "short read on <what>: <path>"
std::vector<unsigned char> read_file(const char* path, const char* what);
// written to a temporary beside `path`, checked, then renamed over it; Error(KX_ERR_IO) and no temporary left otherwise
void write_file_atomic(const std::string& path, const void* data, size_t n);

// the KXHIPW01 image behind `path`: the container itself (header checked), or built from the `.onnx` the reference passes
// *variant (optional): what the file was -- 0 KXHIPW01 container, 1 fp32 ONNX, 2 fp16 / bf16 ONNX, 3 8-bit quantised ONNX,
// 4 4-bit quantised ONNX (3, 4: weights de-quantised), -1 a cached conversion (KOKOROX_KXW_CACHE=1)
std::vector<unsigned char> read_weight_file(const char* path, int* variant = nullptr);
std::vector<unsigned char> import_onnx_bytes(const unsigned char* data, size_t n, int* variant = nullptr);  // ImportError -> Error(KX_ERR_IO)

}  // namespace kx
