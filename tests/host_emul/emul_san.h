// tests/host_emul/emul_san.h -- TEST INFRASTRUCTURE ONLY.
//
// What the main() of every sanitizer program (<family>_emul_san: <family>_emul.cpp under -DAASM_EMUL_SAN_MAIN) does with its files
// and its arrays: read a file whole, as bytes or as int64 words; copy an array into a heap block of EXACTLY its size, converting the
// cells, so that the sanitizer ends the program at the first cell touched outside it; append outputs as int64 words; write a file.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace emul_san {
// the whole file -> data; false: it cannot be opened
inline bool read_bytes(const char *path, std::vector<char> &data) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    return true;
}
// a file of int64 words -> words (the files are padded to whole words: a shorter tail is dropped)
inline bool read_words(const char *path, std::vector<int64_t> &words) {
    std::vector<char> data;
    if (!read_bytes(path, data)) return false;
    words.resize(data.size() / 8);
    if (!words.empty()) std::memcpy(words.data(), data.data(), words.size() * 8);
    return true;
}
// a heap block of exactly n cells of T (one byte where n <= 0), uninitialised; the caller frees it
template <class T> T *block(int64_t n) { return (T *)std::malloc(n > 0 ? (size_t)n * sizeof(T) : 1); }
// ... holding src[0, n), each cell converted to T
template <class T, class S> T *exact(const S *src, int64_t n) {
    T *p = block<T>(n);
    for (int64_t i = 0; i < n; i++) p[i] = (T)src[i];
    return p;
}
// ... holding zeros: an output array
template <class T> T *zeros(int64_t n) {
    T *p = block<T>(n);
    for (int64_t i = 0; i < n; i++) p[i] = (T)0;
    return p;
}
// p[0, n) behind out, as int64 words
template <class T> void put(std::vector<int64_t> &out, const T *p, int64_t n) { for (int64_t i = 0; i < n; i++) out.push_back((int64_t)p[i]); }
inline bool write_bytes(const char *path, const void *data, size_t bytes) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}
inline bool write_words(const char *path, const std::vector<int64_t> &words) { return write_bytes(path, words.data(), words.size() * 8); }
}  // namespace emul_san
