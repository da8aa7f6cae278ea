"""Caller-side mirror of the reference's client layer (src/client.rs) -- SURVEY section 8(f) row f1.

`VectorLiteClient` / `Collection` keep the reference's behaviour: collections by name, `IndexType`
{Flat, HNSW} (HNSW requires a metric, src/client.rs:69-72), ids allocated from an atomic counter that
starts at 0 or at max_id + 1 after a load (:295-315), embedding OUTSIDE the index lock (:353, :395),
string errors of `add`/`delete` re-typed by substring (:334-345, :384-390), metric defaulting to the
index's own metric or Cosine (:143-155).  The index underneath is the GPU one.  Embedding models are
out of scope: `embedding_function` is any object with `generate_embedding(text) -> list[float]` and
`dimension()` (trait EmbeddingFunction, src/embeddings.rs:135-141).
"""
from __future__ import annotations

import enum
import itertools
import threading
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence

from . import (DimensionMismatch, FlatIndex, HNSWIndex, IndexOpError, SearchResult, SimilarityMetric, Vector,
               VectorLiteError)


class IndexType(enum.Enum):
    Flat = "flat"
    HNSW = "hnsw"


class CollectionAlreadyExists(VectorLiteError):
    pass


class CollectionNotFound(VectorLiteError):
    pass


class MetricRequired(VectorLiteError):
    pass


class DuplicateVectorId(VectorLiteError):
    pass


class VectorNotFound(VectorLiteError):
    pass


@dataclass
class CollectionInfo:
    name: str
    count: int
    is_empty: bool
    dimension: int


class Collection:
    def __init__(self, name: str, index):
        self._name = name
        self.index = index
        mx = index.max_id()
        self._next = itertools.count(0 if mx is None else mx + 1)  # src/client.rs:297-308
        self._next_peek = 0 if mx is None else mx + 1
        self._lock = threading.Lock()  # guards the counter only; the index has its own RW discipline

    def name(self) -> str:
        return self._name

    def next_id(self) -> int:
        return self._next_peek

    def _alloc_id(self) -> int:
        with self._lock:
            i = next(self._next)
            self._next_peek = i + 1
            return i

    def add_text_with_metadata(self, text: str, metadata: Optional[Any], embedding_function) -> int:
        vid = self._alloc_id()
        embedding = embedding_function.generate_embedding(text)  # outside any index lock
        try:
            self.index.add(Vector(id=vid, values=embedding, text=text, metadata=metadata))
        except IndexOpError as e:
            msg = str(e)
            if "dimension" in msg:
                raise DimensionMismatch(self.index.dimension(), len(embedding)) from e
            if "already exists" in msg:
                raise DuplicateVectorId(f"Vector ID {vid} already exists") from e
            raise VectorLiteError(msg) from e
        return vid

    def add_text(self, text: str, embedding_function) -> int:
        return self.add_text_with_metadata(text, None, embedding_function)

    def delete(self, id: int) -> None:
        try:
            self.index.delete(id)
        except IndexOpError as e:
            if "does not exist" in str(e):
                raise VectorNotFound(f"Vector ID {id} not found") from e
            raise VectorLiteError(str(e)) from e

    def delete_many(self, ids) -> int:
        """`for id in ids: delete(id)` in one index call (a document's chunks, a tombstone list); returns the rows removed.
        An HNSW collection stops at the first id it does not hold, as the loop would."""
        try:
            return self.index.delete_many(ids)
        except IndexOpError as e:
            if "does not exist" in str(e):
                raise VectorNotFound(str(e).replace("does not exist", "not found")) from e
            raise VectorLiteError(str(e)) from e

    def update_text(self, id: int, text: str, metadata: Optional[Any], embedding_function) -> None:
        """Re-embed a stored chunk in place (a changed text, a corrected vector): the row keeps its id and its position, and
        filters made earlier stay resolved (FlatIndex.update).  Flat collections only.  The index row and the side table of
        text and metadata change under one lock: two updates of one id leave the values and the text of the same call."""
        embedding = embedding_function.generate_embedding(text)  # outside any lock
        try:
            with self._lock:
                self.index.update(Vector(id=id, values=embedding, text=text, metadata=metadata))
        except IndexOpError as e:
            if "does not exist" in str(e):
                raise VectorNotFound(f"Vector ID {id} not found") from e
            raise VectorLiteError(str(e)) from e

    def search_text(self, query_text: str, k: int, similarity_metric: SimilarityMetric, embedding_function,
                    where: Optional[Callable[[Any], bool]] = None) -> List[SearchResult]:
        """`where`: a predicate on a row's metadata; only rows for which it holds are ranked (an exact filtered search
        over the ids whose metadata matches -- flat collections)."""
        embedding = embedding_function.generate_embedding(query_text)
        if where is None:
            return self.index.search(embedding, k, similarity_metric)
        ids = [i for i, (_text, md) in list(self.index._meta.items()) if where(md)]
        return self.index.search(embedding, k, similarity_metric, filter=ids)

    def search_texts(self, texts: Sequence[str], k: int, similarity_metric: SimilarityMetric, embedding_function,
                     wheres: Optional[Sequence[Optional[Callable[[Any], bool]]]] = None) -> List[List[SearchResult]]:
        """search_text for a batch of requests, each with its own optional predicate (`wheres[i]`, None: no filter) -- what
        a server does with the requests of different users that arrive together.  Entry i is exactly
        search_text(texts[i], ..., where=wheres[i]).  Predicates that select the same id set share one filter; the
        filtered queries go through one FlatIndex.search_batch(filters=...), the others through one search_batch."""
        texts = list(texts)
        wheres = [None] * len(texts) if wheres is None else list(wheres)
        if len(wheres) != len(texts):
            raise ValueError("`wheres` must hold one predicate (or None) per text")
        embeddings = [embedding_function.generate_embedding(t) for t in texts]
        if not isinstance(self.index, FlatIndex):  # no batched filters there: one by one
            return [self.index.search(e, k, similarity_metric) if w is None else
                    self.index.search(e, k, similarity_metric, filter=[i for i, (_t, md) in list(self.index._meta.items()) if w(md)])
                    for e, w in zip(embeddings, wheres)]
        out: List[List[SearchResult]] = [[] for _ in texts]

        def fill(rows, ids, scores, n):
            for r, qi in enumerate(rows):
                for i, s in zip(ids[r, :int(n[r])].tolist(), scores[r, :int(n[r])].tolist()):
                    text, md = self.index._meta.get(i, ("", None))
                    out[qi].append(SearchResult(id=i, score=s, text=text, metadata=md))

        plain = [qi for qi, w in enumerate(wheres) if w is None]
        if plain:
            fill(plain, *self.index.search_batch([embeddings[qi] for qi in plain], k, similarity_metric))
        picky = [qi for qi, w in enumerate(wheres) if w is not None]
        if picky:
            meta = list(self.index._meta.items())
            by_ids: Dict[tuple, Any] = {}  # id set -> its filter
            try:
                filters = []
                for qi in picky:
                    key = tuple(sorted(i for i, (_text, md) in meta if wheres[qi](md)))
                    if key not in by_ids:
                        by_ids[key] = self.index.make_filter(key)
                    filters.append(by_ids[key])
                fill(picky, *self.index.search_batch([embeddings[qi] for qi in picky], k, similarity_metric, filters=filters))
            finally:
                for f in by_ids.values():
                    f.close()
        return out

    def search_text_mmr(self, query_text: str, k: int, similarity_metric: SimilarityMetric, embedding_function,
                        fetch_k: int = 20, lambda_mult: float = 0.5) -> List[SearchResult]:
        """search_text with diversified results: maximal marginal relevance over the best fetch_k chunks (flat
        collections; FlatIndex.search_mmr)."""
        embedding = embedding_function.generate_embedding(query_text)
        return self.index.search_mmr(embedding, k, fetch_k, lambda_mult, similarity_metric)

    def get_vector(self, id: int) -> Optional[Vector]:
        return self.index.get_vector(id)

    def get_info(self) -> CollectionInfo:
        return CollectionInfo(self._name, len(self.index), self.index.is_empty(), self.index.dimension())

    def save_to_file(self, path: str) -> None:
        from . import persistence
        persistence.save_collection_to_file(self._name, self.index, path)

    @classmethod
    def load_from_file(cls, path: str, device: int = 0) -> "Collection":
        from . import persistence
        name, index = persistence.load_collection_from_file(path, device=device)
        return cls(name, index)


class VectorLiteClient:
    def __init__(self, embedding_function, device: int = 0):
        self.embedding_function = embedding_function
        self.device = device
        self.collections: Dict[str, Collection] = {}

    def create_collection(self, name: str, index_type: IndexType, metric: Optional[SimilarityMetric] = None) -> None:
        if name in self.collections:
            raise CollectionAlreadyExists(name)
        dim = self.embedding_function.dimension()
        if index_type == IndexType.Flat:
            index = FlatIndex(dim, device=self.device)
        else:
            if metric is None:
                raise MetricRequired("HNSW requires a similarity metric")
            index = HNSWIndex(dim, metric, device=self.device)
        self.collections[name] = Collection(name, index)

    def add_collection(self, collection: Collection) -> None:
        if collection.name() in self.collections:
            raise CollectionAlreadyExists(collection.name())
        self.collections[collection.name()] = collection

    def get_collection(self, name: str) -> Optional[Collection]:
        return self.collections.get(name)

    def list_collections(self) -> List[str]:
        return list(self.collections.keys())

    def has_collection(self, name: str) -> bool:
        return name in self.collections

    def delete_collection(self, name: str) -> None:
        if self.collections.pop(name, None) is None:
            raise CollectionNotFound(name)

    def _get(self, name: str) -> Collection:
        c = self.collections.get(name)
        if c is None:
            raise CollectionNotFound(name)
        return c

    def add_text_to_collection(self, collection_name: str, text: str, metadata: Optional[Any] = None) -> int:
        return self._get(collection_name).add_text_with_metadata(text, metadata, self.embedding_function)

    def search_text_in_collection(self, collection_name: str, query_text: str, k: int,
                                  similarity_metric: Optional[SimilarityMetric] = None,
                                  where: Optional[Callable[[Any], bool]] = None) -> List[SearchResult]:
        c = self._get(collection_name)
        if similarity_metric is None:  # src/client.rs:143-155
            similarity_metric = c.index.metric() if isinstance(c.index, HNSWIndex) else SimilarityMetric.Cosine
        return c.search_text(query_text, k, similarity_metric, self.embedding_function, where=where)

    def search_texts_in_collection(self, collection_name: str, query_texts: Sequence[str], k: int,
                                   similarity_metric: Optional[SimilarityMetric] = None,
                                   wheres: Optional[Sequence[Optional[Callable[[Any], bool]]]] = None) -> List[List[SearchResult]]:
        """search_text_in_collection for a batch of requests, each with its own optional `where` (Collection.search_texts)."""
        c = self._get(collection_name)
        if similarity_metric is None:
            similarity_metric = c.index.metric() if isinstance(c.index, HNSWIndex) else SimilarityMetric.Cosine
        return c.search_texts(query_texts, k, similarity_metric, self.embedding_function, wheres=wheres)

    def delete_from_collection(self, collection_name: str, id: int) -> None:
        self._get(collection_name).delete(id)

    def update_text_in_collection(self, collection_name: str, id: int, text: str, metadata: Optional[Any] = None) -> None:
        self._get(collection_name).update_text(id, text, metadata, self.embedding_function)

    def get_vector_from_collection(self, collection_name: str, id: int) -> Optional[Vector]:
        return self._get(collection_name).get_vector(id)

    def get_collection_info(self, collection_name: str) -> CollectionInfo:
        return self._get(collection_name).get_info()
