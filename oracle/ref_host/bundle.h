// bundle.h -- the request / result files of the stand-alone reference programs (driver.cpp, driver_icp.cpp).
// TEST INFRASTRUCTURE ONLY; this project's own code.
//
// Files: "RHB1", int32 count, then per array: char name[24], int32 dtype (0 u8, 1 i32, 2 f32, 3 f64), int32 ndim,
// int64 shape[4], the data, zero padding to 8 bytes (oracle/ref_host/__init__.py writes and reads them with numpy).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

struct Arr {
    int dtype = 0;
    std::vector<int64_t> shape;
    std::vector<uint8_t> data;
    size_t count() const { size_t n = 1; for (int64_t s : shape) n *= (size_t)s; return n; }
};
const size_t kElem[4] = {1, 4, 4, 8};
template <typename T> struct DType;
template <> struct DType<uint8_t> { static const int v = 0; };
template <> struct DType<int32_t> { static const int v = 1; };
template <> struct DType<float> { static const int v = 2; };
template <> struct DType<double> { static const int v = 3; };

struct Bundle {
    std::map<std::string, Arr> arrays;
    std::vector<std::string> order;

    bool has(const std::string& n) const { return arrays.count(n) != 0; }
    const Arr& at(const std::string& n) const {
        auto it = arrays.find(n);
        if (it == arrays.end()) throw std::runtime_error("request lacks `" + n + "`");
        return it->second;
    }
    template <typename T> const T* ptr(const std::string& n, size_t want = 0) const {
        const Arr& a = at(n);
        if (a.dtype != DType<T>::v) throw std::runtime_error("`" + n + "` has the wrong type");
        if (want != 0 && a.count() != want)
            throw std::runtime_error("`" + n + "` has " + std::to_string(a.count()) + " elements, not " + std::to_string(want));
        return reinterpret_cast<const T*>(a.data.data());
    }
    template <typename T> const T* opt(const std::string& n, size_t want = 0) const { return has(n) ? ptr<T>(n, want) : nullptr; }
    size_t count(const std::string& n) const { return at(n).count(); }
    int geti(const std::string& n) const { return *ptr<int32_t>(n, 1); }
    float getf(const std::string& n) const { return *ptr<float>(n, 1); }
    template <typename T> void put(const std::string& n, const T* p, std::vector<int64_t> shape) {
        Arr a;
        a.dtype = DType<T>::v;
        a.shape = shape;
        a.data.resize(a.count() * sizeof(T));
        if (a.count()) std::memcpy(a.data.data(), p, a.data.size());
        if (!arrays.count(n)) order.push_back(n);
        arrays[n] = a;
    }
    template <typename T> void put(const std::string& n, const std::vector<T>& v, std::vector<int64_t> shape) { put(n, v.data(), shape); }
};

Bundle read_bundle(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    Bundle b;
    char magic[4];
    int32_t n = 0;
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RHB1", 4) != 0 || std::fread(&n, 4, 1, f) != 1)
        throw std::runtime_error("not a request file");
    for (int i = 0; i < n; i++) {
        char name[24];
        int32_t dtype, ndim;
        int64_t shape[4];
        if (std::fread(name, 1, 24, f) != 24 || std::fread(&dtype, 4, 1, f) != 1 || std::fread(&ndim, 4, 1, f) != 1 ||
            std::fread(shape, 8, 4, f) != 4 || dtype < 0 || dtype > 3 || ndim < 0 || ndim > 4)
            throw std::runtime_error("bad array header");
        name[23] = 0;
        Arr a;
        a.dtype = dtype;
        a.shape.assign(shape, shape + ndim);
        const size_t bytes = a.count() * kElem[dtype], padded = (bytes + 7) / 8 * 8;
        a.data.resize(padded);
        if (padded && std::fread(a.data.data(), 1, padded, f) != padded) throw std::runtime_error("short array data");
        a.data.resize(bytes);
        b.order.push_back(name);
        b.arrays[name] = a;
    }
    std::fclose(f);
    return b;
}

void write_bundle(const char* path, const Bundle& b) {
    FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error(std::string("cannot write ") + path);
    const int32_t n = (int32_t)b.order.size();
    std::fwrite("RHB1", 1, 4, f);
    std::fwrite(&n, 4, 1, f);
    for (const std::string& name : b.order) {
        const Arr& a = b.arrays.at(name);
        char nm[24] = {};
        std::strncpy(nm, name.c_str(), 23);
        const int32_t dtype = a.dtype, ndim = (int32_t)a.shape.size();
        int64_t shape[4] = {0, 0, 0, 0};
        for (int i = 0; i < ndim; i++) shape[i] = a.shape[i];
        std::fwrite(nm, 1, 24, f);
        std::fwrite(&dtype, 4, 1, f);
        std::fwrite(&ndim, 4, 1, f);
        std::fwrite(shape, 8, 4, f);
        if (!a.data.empty()) std::fwrite(a.data.data(), 1, a.data.size(), f);
        const char zero[8] = {};
        std::fwrite(zero, 1, (8 - a.data.size() % 8) % 8, f);
    }
    std::fclose(f);
}

// A non-null pointer for an empty vector: the launchers hand thrust's data() of an empty vector to the kernels.
template <typename T> T* data_of(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

}  // namespace
